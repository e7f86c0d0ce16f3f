// sf_stream_core.h -- the device code under the stream decoder's kernels (sf_stream.hip): the reader over an item's body, the
// lane-serial block decoder of the count and write passes (stream_decode) and the window step of compose and resolve.
#pragma once
#include "sf_device.h"

#include "sf_inflate_core.h"
#include "sf_members.h"

namespace sf {

namespace {

using namespace inflate;

constexpr uint32_t KF_THREADS = 256;                 // k_stream_find: 4 waves, one nominal chunk each
constexpr uint32_t KS_LANES = 4;                     // k_stream_decode: lanes per workgroup (as k_inflate_tokens)
constexpr uint32_t KS_LDS = KS_LANES * LaneLayout::kBytes;
constexpr uint32_t KR_THREADS = 1024;                // compose / link / resolve: one 32 KiB window in LDS
constexpr uint32_t kWin = 32768;
constexpr uint32_t kPerThread = kWin / KR_THREADS;
constexpr uint32_t kRebase = 1u << 30;

// The reader at body bit `at`: bitpos counts from the byte holding it (rb = that byte's first bit).
struct StreamReader {
  BitReader br;
  uint64_t rb;
  __device__ void open(const uint8_t* src, uint64_t src_n, uint64_t b0, uint64_t body_n, uint64_t at) {
    const uint64_t byte = at >> 3;
    br.open(src, src_n, b0 + byte, b0 + body_n);
    rb = byte * 8;
    br.refill();
    br.drop((uint32_t)(at & 7));
  }
  __device__ uint64_t abs() const { return rb + br.bitpos; }
  __device__ uint32_t rem() const { return br.nbits - br.bitpos; }  // exact while bitpos <= 2^30 + 2^20 (see the header)
};

// A stored block's payload into the plane: `len` bytes at `from` (any address inside the stream) become `len` u16 entries at
// `to` (2-byte aligned).  A head of single entries brings `to` to a 16-byte boundary; then 16 bytes per step: the source as
// aligned dwords, one carried from step to step and funnelled to the source's byte offset, widened to 16 entries and written
// by two 16-byte stores; a tail of single entries.  No dword past the one holding the payload's last byte is loaded (a step
// whose source is dword-aligned repeats its last one instead), so nothing beyond the stream's last dword is read.  The stream's first byte is 4-byte aligned, as BitReader needs it (host
// sources are staged that way, device ones are checked), so that an aligned dword never straddles the end of what d_src promises.
typedef uint32_t Store16 __attribute__((ext_vector_type(4), may_alias));  // (the plane is read back as u16)
__device__ __forceinline__ void copy_stored(uint16_t* __restrict__ to, const uint8_t* __restrict__ from, uint32_t len) {
  uint32_t k = (uint32_t)((0 - reinterpret_cast<uintptr_t>(to)) & 15u) >> 1;
  k = k < len ? k : len;
  for (uint32_t j = 0; j < k; ++j) to[j] = from[j];
  if (len - k >= 16) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(from + k);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const uint32_t sh = 8 * (uint32_t)(a & 3);
    const uint32_t lastw = (uint32_t)((reinterpret_cast<uintptr_t>(from + len - 1) >> 2) - (a >> 2));
    uint32_t carry = w[0], i = 1;
    for (; k + 16 <= len; k += 16) {
      uint32_t d[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j, ++i) {
        const uint32_t nx = w[i < lastw ? i : lastw];
        d[j] = (uint32_t)((((uint64_t)nx << 32) | carry) >> sh);
        carry = nx;
      }
      Store16* o = reinterpret_cast<Store16*>(to + k);
      o[0] = Store16{(d[0] & 0xFFu) | ((d[0] & 0xFF00u) << 8), ((d[0] >> 16) & 0xFFu) | ((d[0] >> 8) & 0xFF0000u),
                        (d[1] & 0xFFu) | ((d[1] & 0xFF00u) << 8), ((d[1] >> 16) & 0xFFu) | ((d[1] >> 8) & 0xFF0000u)};
      o[1] = Store16{(d[2] & 0xFFu) | ((d[2] & 0xFF00u) << 8), ((d[2] >> 16) & 0xFFu) | ((d[2] >> 8) & 0xFF0000u),
                        (d[3] & 0xFFu) | ((d[3] & 0xFF00u) << 8), ((d[3] >> 16) & 0xFFu) | ((d[3] >> 8) & 0xFF0000u)};
    }
  }
  for (; k < len; ++k) to[k] = from[k];
}

// Blocks of one chunk (see the header).  WRITE: the exact rules, and the symbol plane from plane[c.base].
// MEMBERS (a file of gzip members; the body reaches to the file's end): a BFINAL block closes a member, not the chunk.  The lane
// hops (sf_members.h) over the trailer, the zero bytes and the next header and goes on in the next body while the chunk's
// range lasts; final_ is the file's end.  side: the chunk's side row.  The count pass leaves in it how many members the chunk
// closed and where in its output the last of them ended; the write pass finds there where the member open at the chunk's
// start began in the item's output (a match may reach no further back) and the first row of mem that is the chunk's to
// write, one row per member it closes (item: the chunk's item row, for the host to place the rows).
template <bool WRITE, bool MEMBERS>
__device__ void stream_decode(const uint8_t* src, uint64_t src_n, uint64_t b0, uint64_t body_n, StreamChunk& c, uint8_t* m,
                              uint16_t* __restrict__ plane, uint64_t cap, StreamSide* side = nullptr,
                              StreamMember* __restrict__ mem = nullptr, uint32_t item = 0) {
  StreamReader rd;
  rd.open(src, src_n, b0, body_n, c.start);
  BitReader& br = rd.br;
  const uint64_t base = c.base;
  uint64_t pos = 0;
  uint32_t st = kOk, fin = 0;
  uint64_t member0 = 0;               // MEMBERS, WRITE: where the open member began in the item's output
  uint32_t closed = 0, eof = 0;       // MEMBERS: members closed so far, the file's end
  uint64_t closed_at = 0;
  if (MEMBERS && WRITE) member0 = side->at;
  for (;;) {
    if (fin) {
      if (!MEMBERS) break;
      const members::Hop h = members::hop(src, src_n, 8 * b0 + rd.abs());
      if (h.st != kOk && h.src_end == 0) { st = h.st; break; }  // no trailer
      if (WRITE) {
        if (closed >= side->n) { st = kError; break; }  // (the count pass closed fewer: never)
        mem[side->first + closed] = StreamMember{h.src_end, base + pos, h.crc32, h.isize, item, 0u};
        member0 = base + pos;
      }
      ++closed;
      closed_at = pos;
      if (h.end) { eof = 1; break; }
      if (h.st != kOk) { st = h.st; break; }
      rd.open(src, src_n, b0, body_n, 8 * (h.next - b0));
      fin = 0;
    }
    if (rd.abs() >= c.limit) break;
    if (br.bitpos > kRebase) rd.open(src, src_n, b0, body_n, rd.abs());
    if (rd.rem() < 3) { st = kInvalidBlockHeader; break; }
    br.refill();
    fin = br.get(1);
    const uint32_t type = br.get(2);
    if (type == 3) { st = kInvalidBlockHeader; break; }
    if (type == 0) {
      br.drop((8 - (br.bitpos & 7)) & 7);
      if (rd.rem() < 32) { st = kError; break; }
      br.refill();
      const uint32_t len = br.get(16);
      br.refill();
      const uint32_t nlen = br.get(16);
      if ((len ^ nlen) != 0xFFFFu) { st = kNoCompressionLenMismatch; break; }
      if (rd.rem() < 8 * len) { st = kSrcTooSmall; break; }
      const uint32_t rel = br.bitpos >> 3;
      if (WRITE) {
        if (cap - (base + pos) < len) { st = kDstTooSmall; break; }
        if (pos + len > c.out) { st = kError; break; }  // (the count pass saw fewer bytes: never)
        copy_stored(plane + base + pos, src + b0 + (rd.rb >> 3) + rel, len);
      }
      pos += len;
      br.bitpos += 8 * len;
      br.seek(rel + len);
      continue;
    }
    if (type == 1) {
      read_lengths<LaneLayout>(br, m, 1);
      build_tables<LaneLayout, true>(m);
      build_tables<LaneLayout, false>(m);
    } else if ((st = serial_dynamic<LaneLayout>(br, m)) != kOk) {
      break;
    }
    for (;;) {
      if (br.bitpos > kRebase) rd.open(src, src_n, b0, body_n, rd.abs());
      br.refill();
      uint32_t sym;
      const uint32_t l = decode_symbol<LaneLayout, true>(m, br, sym);
      if (l == 0 || l > rd.rem()) { st = kInvalidLitOrLen; break; }
      br.drop(l);
      if (sym < 256) {
        if (WRITE) {
          if (base + pos >= cap) { st = kDstTooSmall; break; }
          if (pos >= c.out) { st = kError; break; }
          plane[base + pos] = (uint16_t)sym;
        }
        ++pos;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) { st = kInvalidLitOrLen; break; }
      uint32_t lbase, lextra;
      length_info(sym, lbase, lextra);
      if (rd.rem() < lextra) { st = kError; break; }
      const uint32_t len = lbase + br.get(lextra);
      br.refill();
      uint32_t dsym;
      const uint32_t dl = decode_symbol<LaneLayout, false>(m, br, dsym);
      if (dl == 0 || dl > rd.rem()) { st = kInvalidDistance; break; }
      br.drop(dl);
      if (dsym > 29) { st = kInvalidLitOrLen; break; }
      uint32_t dbase, dextra;
      distance_info(dsym, dbase, dextra);
      if (rd.rem() < dextra) { st = kError; break; }
      const uint32_t dist = dbase + br.get(dextra);
      if (WRITE) {
        if (dist > base + pos - member0) { st = kInvalidDistance; break; }
        if (cap - (base + pos) < len) { st = kDstTooSmall; break; }
        if (pos + len > c.out) { st = kError; break; }
        uint16_t* to = plane + base + pos;
        if (dist <= pos) {
          const uint16_t* from = to - dist;
          for (uint32_t k = 0; k < len; ++k) to[k] = from[k];
        } else {
          // window bytes first (marker k: byte k of the 32 KiB before O_i), then the chunk's own
          const int64_t q = (int64_t)pos - (int64_t)dist;
          for (uint32_t k = 0; k < len; ++k) {
            const int64_t p = q + k;
            to[k] = p < 0 ? (uint16_t)(0x8000u | (uint32_t)(kWin + p)) : plane[base + (uint64_t)p];
          }
        }
      }
      pos += len;
    }
    if (st != kOk) break;
  }
  c.end = rd.abs();
  c.status = st;
  c.final_ = MEMBERS ? eof : fin;
  if (!WRITE) c.out = pos;
  if (MEMBERS && !WRITE) *side = StreamSide{closed_at, closed, 0u};
}

// T <- the window after chunk c, from T = the window before it (entries: literal bytes, or 0x8000 | k, entry k of a base window)
__device__ __forceinline__ void window_step(uint16_t* T, const uint16_t* __restrict__ plane, const StreamChunk& c) {
  uint16_t v[kPerThread];
#pragma unroll
  for (uint32_t r = 0; r < kPerThread; ++r) {
    const uint32_t j = r * KR_THREADS + threadIdx.x;
    if (c.out + j < kWin) {
      v[r] = T[c.out + j];
    } else {
      const uint16_t x = plane[c.base + c.out + j - kWin];
      v[r] = x < 256 ? x : T[x & 0x7FFFu];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kPerThread; ++r) T[r * KR_THREADS + threadIdx.x] = v[r];
  __syncthreads();
}

}  // namespace

}  // namespace sf
