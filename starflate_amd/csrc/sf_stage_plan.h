// sf_stage_plan.h -- the host-buffer entry points' way through one pinned staging buffer: `count` items lie packed in a device
// buffer, item i at bytes [off[i], off[i] + len[i]) of it (off ascending, the ranges disjoint: pack_layout), and the packed
// layout [0, total) moves in pieces of at most `piece` bytes, because the pinned buffer holds one piece.  An item may straddle any
// number of pieces.  Also here, next to the 16-byte rounding: Carve, which lays the arrays of one scratch buffer out.  Plain C++,
// no HIP: the copy between the staging and the device is the caller's (`xfer`), so the tests compile these loops for the host
// as well (tests/cpp/stage_plan_host.cpp, tests/cpp/stage_layout_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

namespace sf {
namespace stage {

// The packed layout itself: items lie 16 bytes aligned (the device paths' alignment rules hold for every item of the staging).
inline uint64_t al16(uint64_t b) { return (b + 15) / 16 * 16; }

// One buffer carved into arrays, piece after piece: add<T>(count) is the offset of an array of `count` T -- always a multiple of
// 16, whatever the pieces before it hold -- and bytes() what the pieces added so far take.  A host table and its device twin are
// carved once and read with at<T>(base, off) from either base.
struct Carve {
  size_t end = 0;
  template <class T>
  size_t add(size_t count) {
    const size_t off = end;
    end = (size_t)al16(off + count * sizeof(T));
    return off;
  }
  size_t bytes() const { return end; }
  template <class T>
  static T* at(uint8_t* base, size_t off) { return reinterpret_cast<T*>(base + off); }
};

// off[0 .. count] from `count` slot sizes: slot i is [off[i], off[i] + slot[i]), off[0] = 0, every offset a multiple of 16,
// off[count] the bytes the layout takes.  (A slot of no bytes takes none: it shares its offset with the next one.)
inline void pack_layout(const uint64_t* slot, size_t count, uint64_t* off) {
  off[0] = 0;
  for (size_t i = 0; i < count; ++i) off[i + 1] = al16(off[i] + slot[i]);
}

// The items with bytes in piece [p0, p1): f(i, at, in_piece, n) for bytes [at, at + n) of item i, which are bytes
// [in_piece, in_piece + n) of the piece.  first: an item none before which reaches p0 (pieces are visited in order);
// returns that for the next piece.
template <class F>
inline size_t items_in_piece(const uint64_t* len, const uint64_t* off, size_t count, size_t first, uint64_t p0, uint64_t p1, F&& f) {
  while (first < count && off[first] + len[first] <= p0) ++first;
  for (size_t i = first; i < count && off[i] < p1; ++i) {
    const uint64_t a = std::max(p0, off[i]), b = std::min(p1, off[i] + len[i]);
    if (a < b) f(i, a - off[i], a - p0, b - a);
  }
  return first;
}

// Up: every piece of [0, total) is gathered from the items' sources into `stage`, then xfer(p0, n) sends stage[0, n) to
// bytes [p0, p0 + n) of the packed layout (and returns once `stage` may be refilled).  Bytes of a piece that belong to no
// item (alignment gaps) go up as they lie in the staging.  Returns the first non-zero xfer result.
template <class X>
inline int pack_up(uint8_t* stage, uint64_t piece, const void* const* src, const uint64_t* len, const uint64_t* off, size_t count,
                   uint64_t total, X&& xfer) {
  size_t first = 0;
  for (uint64_t p0 = 0; p0 < total; p0 += piece) {
    const uint64_t p1 = std::min(total, p0 + piece);
    first = items_in_piece(len, off, count, first, p0, p1, [&](size_t i, uint64_t at, uint64_t in_piece, uint64_t n) {
      memcpy(stage + in_piece, (const uint8_t*)src[i] + at, n);
    });
    if (int rc = xfer(p0, p1 - p0)) return rc;
  }
  return 0;
}

// Down: for every piece of [0, total) that holds bytes of an item, xfer(p0, n) fetches bytes [p0, p0 + n) of the packed layout
// into stage[0, n), and the items' bytes in it go to their destinations.  len[i] == 0: item i is skipped (a failed item: nothing
// is written to its destination); a piece that holds no other item's bytes is not fetched.
template <class X>
inline int unpack_down(uint8_t* stage, uint64_t piece, void* const* dst, const uint64_t* len, const uint64_t* off, size_t count,
                       uint64_t total, X&& xfer) {
  size_t first = 0;
  for (uint64_t p0 = 0; p0 < total; p0 += piece) {
    const uint64_t p1 = std::min(total, p0 + piece);
    bool any = false;
    first = items_in_piece(len, off, count, first, p0, p1, [&](size_t, uint64_t, uint64_t, uint64_t) { any = true; });
    if (!any) continue;
    if (int rc = xfer(p0, p1 - p0)) return rc;
    items_in_piece(len, off, count, first, p0, p1, [&](size_t i, uint64_t at, uint64_t in_piece, uint64_t n) {
      memcpy((uint8_t*)dst[i] + at, stage + in_piece, n);
    });
  }
  return 0;
}

}  // namespace stage
}  // namespace sf
