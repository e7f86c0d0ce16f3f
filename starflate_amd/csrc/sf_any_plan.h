// sf_any_plan.h -- the index-free batch decoder (sfh_decompress_any_batch*): from the items of a call to its launch batches.
// Plain C++, no HIP: compiled for the host by the tests as well (tests/cpp/any_plan_host.cpp).
//
// An item of out_n output bytes has max(1, ceil(out_n / 32768)) segments (an empty item has one, which decodes to nothing).
// Items that take no part in the decode (take[i] == 0: the wrapper failed, the stream is not indexable, the destination is too
// small) have no segments and no rows.  The segments of the others, item after item, are cut into LAUNCH BATCHES so that the
// token scratch of a call is bounded:
//   * whole items only: a recovered index has no strips, a row of dependent segments may span the whole item;
//   * at most `cap` segments per batch;
//   * an item larger than the cap runs alone, and the item behind it opens a new batch.
// A batch is a run of the call's items [item0, item1) and of its segment rows [row0, row0 + nseg).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace sf {
namespace aplan {

constexpr uint64_t kSegBytes = 32768;

struct Batch {
  size_t item0, item1;  // the call's items it covers (those that take no part included)
  uint32_t row0, nseg;  // its rows in the call's segment table
  uint32_t nitems;      // items of it that take part
};
struct Plan {
  std::vector<Batch> batches;
  uint32_t nseg = 0;    // of the call
  uint32_t nitems = 0;  // items that take part
  uint32_t widest = 0;  // segments of the largest launch batch
};

inline uint32_t segments_of(uint64_t out_n) { return out_n ? (uint32_t)((out_n + kSegBytes - 1) / kSegBytes) : 1u; }

// take: null (every item takes part), or per item 0 / 1; cap >= 1; the call's segments fit 32 bits (the callers check both)
inline void plan_batches(size_t count, const uint64_t* out_n, const uint8_t* take, uint32_t cap, Plan& P) {
  P = Plan{};
  Batch cur{0, 0, 0, 0, 0};
  auto close = [&](size_t next) {  // the next batch starts with item `next`
    cur.item1 = next;
    if (cur.nseg) {
      P.batches.push_back(cur);
      if (cur.nseg > P.widest) P.widest = cur.nseg;
    }
    cur = Batch{next, next, P.nseg, 0, 0};
  };
  for (size_t i = 0; i < count; ++i) {
    if (take && !take[i]) continue;
    const uint32_t n = segments_of(out_n[i]);
    if ((uint64_t)cur.nseg + n > cap) close(i);
    if (!cur.nseg) cur.item0 = i;  // (a batch is named by its first item that takes part)
    cur.nseg += n;
    ++cur.nitems;
    P.nseg += n;
    ++P.nitems;
    if (n > cap) close(i + 1);
  }
  close(count);
}

}  // namespace aplan
}  // namespace sf
