// sf_inflate_plan.h -- the indexed decoder (sfh_decompress*, sfh_decompress_batch*): from the items of a call to its launch
// batches.  Plain C++, no HIP: compiled for the host by the tests as well (tests/cpp/inflate_plan_host.cpp).
//
// An item of dst_n output bytes has max(1, ceil(dst_n / 32768)) SEGMENTS; its STRIPS are runs of sps = block_bytes / 32768
// segments (0 = 1), the last one shorter: a segment's matches reach back to the start of its strip and no further, so a strip
// is one workgroup of the byte stage.  The call's segments, item after item, are cut into LAUNCH BATCHES of at most `cap`
// segments, so that the token scratch of a call is bounded:
//   * an item of up to max(sps, cap / sps * sps) segments stays whole, in the current batch or, if it does not fit, the next;
//   * a larger one is cut at multiples of that number into batches of its own -- whole strips, so the cut does not change its
//     strips -- and the item behind it starts a new batch;
//   * a batch is larger than the cap only when it is one strip that alone is.
// A batch is a run of the call's segments, so it is named by its first one: item, segment of the item, row and strip in the
// call's tables.  for_rows() walks a batch's strips and segments in table order; nothing per segment is stored.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace sf {
namespace iplan {

constexpr uint64_t kSegBytes = 32768;

struct Batch {
  uint32_t row0, nseg;       // its rows in the call's segment table
  uint32_t strip0, nstrips;  // its rows in the call's strip table
  size_t item0;              // the item of its first segment
  uint32_t k0;               // ... and that segment's number in the item (a multiple of the item's sps)
};
struct Plan {
  std::vector<Batch> batches;
  uint32_t nseg = 0, nstrips = 0;  // of the call
  uint32_t widest = 0;             // segments of the largest launch batch
};

inline uint32_t segments_of(uint64_t dst_n) { return dst_n ? (uint32_t)((dst_n + kSegBytes - 1) / kSegBytes) : 1u; }
inline uint32_t sps_of(const uint32_t* block_bytes, size_t i) {
  return (block_bytes && block_bytes[i]) ? (uint32_t)(block_bytes[i] / kSegBytes) : 1u;
}
// segment k of an item: its output bytes, and the bytes of its strip in front of it
inline uint32_t seg_out_n(uint64_t dst_n, uint32_t k) {
  const uint64_t ob = (uint64_t)k * kSegBytes;
  return dst_n > ob ? (uint32_t)(dst_n - ob < kSegBytes ? dst_n - ob : kSegBytes) : 0u;
}
inline uint32_t seg_hist(uint32_t k, uint32_t sps) { return (k % sps) * (uint32_t)kSegBytes; }

// block_bytes: null, or per item 0 / a multiple of 32768; cap >= 1; the call's segments fit 32 bits (the callers check both)
inline void plan_batches(size_t count, const uint64_t* dst_n, const uint32_t* block_bytes, uint32_t cap, Plan& P) {
  P = Plan{};
  Batch cur{0, 0, 0, 0, 0, 0};
  auto close = [&](size_t item, uint32_t k) {  // the next batch starts with segment k of `item`
    if (cur.nseg) {
      P.batches.push_back(cur);
      if (cur.nseg > P.widest) P.widest = cur.nseg;
    }
    cur = Batch{P.nseg, 0, P.nstrips, 0, item, k};
  };
  for (size_t i = 0; i < count; ++i) {
    const uint32_t nseg = segments_of(dst_n[i]), sps = sps_of(block_bytes, i);
    const uint32_t piece = sps > cap / sps * sps ? sps : cap / sps * sps;
    if (nseg > piece || (uint64_t)cur.nseg + nseg > cap) close(i, 0);
    for (uint32_t k0 = 0; k0 < nseg; k0 += piece) {
      if (k0) close(i, k0);
      const uint32_t n = nseg - k0 < piece ? nseg - k0 : piece, ns = (n + sps - 1) / sps;
      cur.nseg += n;
      cur.nstrips += ns;
      P.nseg += n;
      P.nstrips += ns;
    }
    if (nseg > piece) close(i + 1, 0);
  }
  close(count, 0);
}

// Batch B in table order: strip(first segment counted from the batch's first, segments) for every strip, each followed by
// seg(item, k) for its segments.
template <class FS, class FG>
inline void for_rows(const Batch& B, const uint64_t* dst_n, const uint32_t* block_bytes, FS&& strip, FG&& seg) {
  uint32_t done = 0, k = B.k0;
  for (size_t i = B.item0; done < B.nseg; ++i, k = 0) {
    const uint32_t sps = sps_of(block_bytes, i), left = segments_of(dst_n[i]) - k;
    const uint32_t k1 = k + (B.nseg - done < left ? B.nseg - done : left);
    while (k < k1) {
      const uint32_t n = k1 - k < sps ? k1 - k : sps;
      strip(done, n);
      for (uint32_t j = 0; j < n; ++j) seg(i, k + j);
      k += n;
      done += n;
    }
  }
}

}  // namespace iplan
}  // namespace sf
