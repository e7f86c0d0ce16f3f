// sf_range_plan.h -- random access (sfh_decompress_range*): from byte ranges of one indexed stream's output to the
// descriptor rows of the decoder's launch batches.  Plain C++, no HIP: compiled for the host by the tests as well
// (tests/cpp/range_plan_host.cpp).
//
// A range [off, off + len) of the output lies in the segments off / 32768 .. (off + len - 1) / 32768.  A segment's matches
// may reach back to the start of its strip (block_bytes of output) and no further, so what has to be decoded for the range --
// its DECODE SPAN -- starts with the first segment of the strip that holds `off` and ends with the segment that holds the
// range's last byte.  Every segment of the span is one ROW: its number in the stream, the bytes of history in front of it,
// and a write window [lo, hi) inside its 32 KiB: the part of it that belongs to the range (empty: the segment is resolved in
// LDS only, for the ones behind it).  Byte lo of the row goes to byte dst_off of the range's destination.
// The rows are cut into STRIPS (one workgroup of the byte stage each; the first strip of a span ends where the stream's strip
// ends, the later ones are whole strips, the last one ends with the range) and the strips into LAUNCH BATCHES of at most
// `cap` rows, so that the token scratch of a call is bounded (a strip larger than the cap is a batch of its own).  A range
// is decoded by itself: two ranges in one strip have a span each.  A range of no bytes has no rows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sf_stage_plan.h"

namespace sf {
namespace range {

constexpr uint64_t kSegBytes = 32768;
constexpr uint64_t kMaxRows = 0x7FFFFFFFull;  // rows of one call
constexpr uint64_t kMaxTotal = 1ull << 44;    // output bytes of a stream (as sfh_decompress_device)

struct Row {
  uint64_t seg;      // the segment's number in the stream
  uint64_t dst_off;  // where its byte `lo` goes in the range's destination
  uint32_t range;    // its range
  uint32_t out_n;    // bytes the segment produces (32768, the stream's last one its remainder)
  uint32_t hist;     // bytes of its strip in front of it
  uint32_t lo, hi;   // write window inside the segment; lo == hi: nothing of it is written
};
struct Span {        // per range
  uint64_t first_seg;
  uint32_t row0, nrows;  // its rows in Plan::rows (consecutive, in stream order)
};
struct Strip {       // per workgroup of the byte stage
  uint32_t row0;     // its first row, counted from its launch batch's first row
  uint32_t nrows;
};
struct Batch {
  uint32_t row0, nrows;      // its rows in Plan::rows
  uint32_t strip0, nstrips;  // its strips in Plan::strips
};
struct Plan {
  std::vector<Row> rows;
  std::vector<Span> spans;
  std::vector<Strip> strips;
  std::vector<Batch> batches;
  uint32_t widest = 0;  // rows of the largest launch batch
};

enum : int { kPlanOk = 0, kPlanBadArg = -1, kPlanTooMany = -2 };

inline uint64_t segments_of(uint64_t total_n) { return total_n ? (total_n + kSegBytes - 1) / kSegBytes : 1; }

// block_bytes: 0 (= 32768) or a multiple of 32768; every range inside [0, total_n].  The rows of the call are counted before
// anything is allocated (kPlanTooMany above kMaxRows).  cap: rows per launch batch (>= 1).
inline int plan_ranges(uint64_t total_n, uint32_t block_bytes, size_t count, const uint64_t* offsets, const uint64_t* lengths,
                       uint32_t cap, Plan& P) {
  P = Plan{};
  if (block_bytes % kSegBytes || total_n > kMaxTotal || cap == 0 || (count && (!offsets || !lengths))) return kPlanBadArg;
  const uint64_t sps = block_bytes ? block_bytes / kSegBytes : 1;
  uint64_t nrows = 0;
  for (size_t r = 0; r < count; ++r) {
    if (offsets[r] > total_n || lengths[r] > total_n - offsets[r]) return kPlanBadArg;
    if (!lengths[r]) continue;
    const uint64_t first = offsets[r] / kSegBytes / sps * sps, last = (offsets[r] + lengths[r] - 1) / kSegBytes;
    nrows += last - first + 1;
    if (nrows > kMaxRows) return kPlanTooMany;
  }
  P.rows.reserve((size_t)nrows);
  P.spans.resize(count);
  Batch cur{0, 0, 0, 0};
  auto close = [&] {
    if (cur.nrows) {
      P.batches.push_back(cur);
      if (cur.nrows > P.widest) P.widest = cur.nrows;
    }
    cur = Batch{(uint32_t)P.rows.size(), 0, (uint32_t)P.strips.size(), 0};
  };
  for (size_t r = 0; r < count; ++r) {
    const uint64_t off = offsets[r], end = off + lengths[r];
    Span& S = P.spans[r];
    S.first_seg = off / kSegBytes / sps * sps;
    S.row0 = (uint32_t)P.rows.size();
    S.nrows = 0;
    if (!lengths[r]) continue;
    const uint64_t last = (end - 1) / kSegBytes;
    for (uint64_t g0 = S.first_seg; g0 <= last; g0 += sps) {  // strip by strip
      const uint64_t g1 = g0 + sps - 1 < last ? g0 + sps - 1 : last;
      const uint32_t n = (uint32_t)(g1 - g0 + 1);
      if (cur.nrows && (uint64_t)cur.nrows + n > cap) close();
      P.strips.push_back(Strip{cur.nrows, n});
      ++cur.nstrips;
      for (uint64_t g = g0; g <= g1; ++g) {
        const uint64_t b = g * kSegBytes;  // the segment's first output byte
        Row w;
        w.seg = g;
        w.range = (uint32_t)r;
        w.out_n = (uint32_t)(total_n - b < kSegBytes ? total_n - b : kSegBytes);
        w.hist = (uint32_t)((g - g0) * kSegBytes);
        const uint64_t lo = off > b ? off : b, hi = end < b + w.out_n ? end : b + w.out_n;
        w.lo = lo < hi ? (uint32_t)(lo - b) : 0u;
        w.hi = lo < hi ? (uint32_t)(hi - b) : 0u;
        w.dst_off = lo < hi ? lo - off : 0;
        P.rows.push_back(w);
      }
      cur.nrows += n;
      S.nrows += n;
    }
  }
  close();
  return kPlanOk;
}

// The host-buffer call uploads, per decode span, only the piece of the stream its rows read: from the smallest to the largest
// of the span's index entries (index[first_seg .. first_seg + nrows]), clipped to src_n and rounded out to 16 bytes.  A damaged
// index cannot send a row outside its piece: a row reads from its first entry on, and only when its second entry is not above
// the bytes readable.  A span without rows has the empty piece at 0.
struct Piece {
  uint64_t lo, n;  // bytes [lo, lo + n) of the stream; lo a multiple of 16
};
inline Piece source_piece(const Span& S, const uint64_t* index, uint64_t src_n) {
  uint64_t lo = 0, hi = 0;
  if (S.nrows) {
    lo = hi = index[S.first_seg];
    for (uint32_t k = 1; k <= S.nrows; ++k) {
      const uint64_t e = index[S.first_seg + k];
      lo = e < lo ? e : lo;
      hi = e > hi ? e : hi;
    }
  }
  lo = (lo < src_n ? lo : src_n) / 16 * 16;
  hi = stage::al16(hi < src_n ? hi : src_n);
  return Piece{lo, (hi < src_n ? hi : src_n) - lo};
}

}  // namespace range
}  // namespace sf
