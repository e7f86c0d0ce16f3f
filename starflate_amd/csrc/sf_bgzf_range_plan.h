// sf_bgzf_range_plan.h -- BGZF random access (sfh_decompress_bgzf_ranges*): from byte ranges of a BGZF file's output to the
// decoder's rows, and the virtual offsets of tabix / BAI indexes.  Plain C++, no HIP, host and device: the kernels of
// sf_bgzf.hip (k_bgzf_range_spans, k_bgzf_range_rows) and the host-buffer call of sf_capi.hip plan with the same functions,
// and the tests compile them for the host (tests/cpp/bgzf_range_plan_host.cpp).
//
// The index is the walk's (sf_bgzf_plan.h): member_off[0 .. members] and out_off[0 .. members], member i holding output
// bytes [out_off[i], out_off[i + 1]).  Members have no fixed size, so the member of an output byte is a binary search in
// out_off.  A member is its own strip -- no match reaches before it -- so a range's DECODE SPAN is exactly the members it
// touches, first .. last, every one a ROW of one segment in a strip of one:
//   first = the smallest i with out_off[i + 1] > offset
//   last  = the smallest j with out_off[j + 1] >= offset + length
// Empty members between the two belong to the span (they decode to 0 bytes); empty members in front of `first` and behind
// `last` do not.  A range of 0 bytes has no rows.  Row k of a range is member first + k with a write window [lo, hi) inside
// the member's out_n = out_off[i + 1] - out_off[i] bytes -- the part of it that belongs to the range -- and byte lo goes to byte
// dst_off of the range's destination.  The rows of a call, range after range, are cut into LAUNCH BATCHES of `per` rows
// (batch_chunks on narrow rows, bgzf::wide_batch(batch_chunks) on wide ones); a span may cross a batch boundary, because its
// rows depend on nothing in front of them, and row g is strip g % per of its batch.
//
// What a range call verifies, per member of the span: the gzip wrapper (gzip_head), that its ISIZE equals its indexed size,
// and that the body decodes to exactly that many bytes.  NO checksum: a member's decoded bytes never reach global memory as a
// whole, so there is nothing to verify a CRC-32 against.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sf_bgzf_plan.h"

namespace sf {
namespace bgzf {

constexpr uint64_t kMaxRangeRows = 0x7FFFFFFFull;  // rows of one call
constexpr uint64_t kNoOffset = ~0ull;              // an invalid virtual offset's slot

// the smallest i in [0, members) with a[i + 1] > x (STRICT) or a[i + 1] >= x; members when there is none.  Binary.
template <bool STRICT>
SF_BGZF_HD uint32_t first_reaching(const uint64_t* a, uint32_t members, uint64_t x) {
  uint32_t lo = 0, hi = members;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (STRICT ? a[mid + 1] > x : a[mid + 1] >= x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

struct Span {
  uint32_t first, rows;
};
// rows == 0: a range of no bytes -- or one the index does not hold (it ends behind out_off[members], or the index is not
// ascending there): range_inside() tells the two apart
SF_BGZF_HD bool range_inside(const uint64_t* out_off, uint32_t members, uint64_t offset, uint64_t length) {
  const uint64_t total = out_off[members];
  return offset <= total && length <= total - offset;
}
SF_BGZF_HD Span span_of(const uint64_t* out_off, uint32_t members, uint64_t offset, uint64_t length) {
  if (!length || !range_inside(out_off, members, offset, length)) return Span{0, 0};
  const uint32_t first = first_reaching<true>(out_off, members, offset);
  const uint32_t last = first_reaching<false>(out_off, members, offset + length);
  if (first >= members || last >= members || last < first) return Span{0, 0};  // (an index that does not ascend)
  return Span{first, last - first + 1};
}

struct RangeRow {
  uint32_t member;   // first + k
  uint32_t out_n;    // the bytes it holds by the index (above 65536: clamped to 0xFFFFFFFF by the subtraction's width)
  uint32_t lo, hi;   // write window inside them; lo == hi: nothing of it is written
  uint64_t dst_off;  // where byte lo goes in the range's destination
};
SF_BGZF_HD RangeRow row_of(const uint64_t* out_off, uint32_t first, uint32_t k, uint64_t offset, uint64_t length) {
  const uint32_t i = first + k;
  const uint64_t b = out_off[i], e = out_off[i + 1], end = offset + length;
  const uint64_t on = e >= b ? e - b : 0;
  const uint64_t lo = offset > b ? offset : b, hi = end < e ? end : e;
  RangeRow w;
  w.member = i;
  w.out_n = on > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)on;
  const bool any = lo < hi && hi - b <= 0xFFFFFFFFull;
  w.lo = any ? (uint32_t)(lo - b) : 0u;
  w.hi = any ? (uint32_t)(hi - b) : 0u;
  w.dst_off = any ? lo - offset : 0;
  return w;
}

// the cut into launch batches of `per` rows (>= 1): batch b holds rows [b * per, b * per + batch_rows(b))
SF_BGZF_HD uint64_t range_batches(uint64_t rows, uint32_t per) { return (rows + per - 1) / per; }
SF_BGZF_HD uint32_t range_batch_rows(uint64_t rows, uint32_t per, uint64_t b) {
  const uint64_t left = rows - b * per;
  return (uint32_t)(left < per ? left : per);
}
SF_BGZF_HD uint32_t rows_per_batch(uint32_t batch_chunks, bool wide) { return wide ? wide_batch(batch_chunks) : (batch_chunks ? batch_chunks : 1u); }

// The host-buffer call uploads, per decode span, only the members' bytes [member_off[first], member_off[first + rows]),
// clipped to src_n and rounded out to 16 bytes (so that the row's file base keeps the bit reader's alignment).  An index that
// disagrees with the file cannot send a row outside its piece: k_bgzf_range_rows places every member inside [lo, lo + n)
// before it reads a byte of it.  A span without rows has the empty piece at 0.
struct RangePiece {
  uint64_t lo, n;  // bytes [lo, lo + n) of the file; lo a multiple of 16
};
SF_BGZF_HD RangePiece range_piece(const uint64_t* member_off, Span S, uint64_t src_n) {
  if (!S.rows) return RangePiece{0, 0};
  uint64_t lo = member_off[S.first], hi = member_off[S.first + S.rows];
  lo = (lo < src_n ? lo : src_n) / 16 * 16;
  hi = hi < src_n ? hi : src_n;
  hi = (hi + 15) / 16 * 16;
  hi = hi < src_n ? hi : src_n;
  return RangePiece{lo, hi > lo ? hi - lo : 0};
}

// ---- virtual offsets: v = coffset << 16 | uoffset, coffset a member's first byte in the file, uoffset a byte of its output ----
// v -> out_off[i] + uoffset where member_off[i] == coffset (a binary search; of several members at one coffset -- there are
// none in a file that parses -- the first) and uoffset <= out_n_i; coffset == member_off[members] with uoffset == 0 -> total_n;
// anything else -> kNoOffset.
SF_BGZF_HD uint64_t voffset_to_offset(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, uint64_t v) {
  const uint64_t c = v >> 16, u = v & 0xFFFFu;
  uint32_t lo = 0, hi = members;  // the smallest i in [0, members] with member_off[i] >= c
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (member_off[mid] >= c) hi = mid;
    else lo = mid + 1;
  }
  if (member_off[lo] != c) return kNoOffset;
  if (lo == members) return u == 0 ? out_off[members] : kNoOffset;
  return u <= out_off[lo + 1] - out_off[lo] ? out_off[lo] + u : kNoOffset;
}
// o -> the member that HOLDS byte o (span_of's `first` rule: never an empty member for a byte that exists) and o's place in
// it; o == total_n -> member_off[members] << 16; o above total_n, or a coffset that does not fit 48 bits -> kNoOffset.
SF_BGZF_HD uint64_t offset_to_voffset(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, uint64_t o) {
  if (o > out_off[members]) return kNoOffset;
  const uint32_t i = o == out_off[members] ? members : first_reaching<true>(out_off, members, o);
  const uint64_t c = member_off[i], u = i == members ? 0 : o - out_off[i];
  if (c >> 48 || u > 0xFFFFu) return kNoOffset;
  return c << 16 | u;
}

}  // namespace bgzf
}  // namespace sf
