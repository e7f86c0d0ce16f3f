// sf_stream.hip -- raw, zlib or gzip streams (one member each), or files of gzip members, decoded on the GPU with no side information and no flush points
// (sfh_inflate_stream*, sfh_inflate_stream_batch*; DESIGN.md 3a "Streams without flush points").  A call holds one item or
// many; a single stream is a call of one item.  Each kernel reads its item's stream, body (the stream without its wrapper),
// plane, capacity and output from a StreamItem row (sf_device.h).  The body is cut into chunks at speculative block starts, the
// chunks are decoded lane-serially, and a chain rule keeps exactly the serial decoder's block sequence.  The records of all
// items lie in one array, item after item (a record's item: rec_item):
//
//   k_stream_find        A. one wave per nominal chunk start of the call (every S body bytes of an item, S = SFH_STREAM_CHUNK):
//                           the first bit offset before the next nominal start where dynamic_header_candidate or
//                           stored_header_candidate (sf_inflate_core.h) holds, the latter only where the block behind its
//                           payload is a stored one too (stored_run_follows): inside a run of stored blocks.  The last
//                           block of a run is left to the lane that comes through; the Huffman block behind it has its
//                           own candidate if it is a dynamic one.  An item's chunk 0 starts at its body's first bit
//                           whatever its block type.
//   k_stream_decode<0>   B. one lane per record: whole blocks from the chunk's start until the first block end at or beyond the
//                           next chunk's start (an item's last chunk: until BFINAL or an error).  Records the end bit, the
//                           output bytes, BFINAL and the first structural problem.  The checks that need the absolute output
//                           position (distance <= bytes written, dst capacity) wait for the write pass.
//                        C. on the host (sf_stream_chain.h), over each item's slice of the records: chunk i+1 is confirmed when
//                           chunk i is and ended, without BFINAL, exactly on i+1's start.  Every broken link is redecoded from
//                           the end before it, all of a round in parallel; then one lane per item with a broken link follows
//                           the first of them through the run of broken links behind it, and stops at its item's last record.
//   k_stream_decode<1>   D. the confirmed records of a launch batch's items again, with the exact rules now that each chunk's
//                           output offset O_i (an exclusive scan of its item's counts) and the capacity are known.  Every
//                           output byte becomes a u16 in the symbol plane (plane + the item's offset, so a record's base stays
//                           item-relative): a literal byte (< 256), or 0x8000 | k, byte k of the 32 KiB window before O_i.
//   k_stream_compose     F. the window of chunk i+1 is a map of chunk i's tail over chunk i's window.  Per item, groups of
//   k_stream_link           G ~ sqrt(N) chunks compose their maps in parallel (compose, one workgroup per (item, group)), one
//   k_stream_resolve        workgroup per item of more than one group carries the window across its groups (link, N/G steps),
//                           and every group then writes its chunks' final bytes into the item's dst (resolve).
//
// The statuses are the serial decoder's (include/starflate/decompress.hpp): stream_decode follows its checks in its order,
// including where the input runs out.  Dynamic blocks and non-final stored blocks in front of another stored block are candidates
// (a stored block with non-zero padding is not); fixed blocks are not, three header bits being no evidence, so a Z_FIXED
// stream is decoded by one lane: slow, but correct.  A stored block's payload goes into the plane 16 bytes per step (copy_stored).  Bit positions and output counts are 64-bit; the 32-bit BitReader is re-opened before its position passes 2^30.
// Scratch: 2 bytes per output byte (the plane), 64 KiB per group, 60 bytes per nominal chunk.
//
// A file of gzip members (SFH_GZIP_MEMBERS; every item of such a call is one) is ONE body from its first header's end to its
// last byte: where a member's BFINAL block ends, the lane hops over the trailer, the zero bytes and the next header
// (sf_members.h) and decodes on, so chunks, chain and resolve are the single member's.  Three things are added.  Find: a
// nominal chunk's candidate may also be the body start behind a member head whose header ends inside the chunk's range.  The
// side rows (sf_stream_chain.h): the count pass counts the members each chunk closes, the host's scan gives each chunk its
// first member row and the output offset at which the member open at its start began, and the write pass refuses a distance
// that reaches before that offset -- so no window marker leaves its member, and compose, link and resolve stay as they are --
// and writes one member row per member it closes: the trailer's CRC-32 and ISIZE, which the host then checks per member.
// Scratch: 16 bytes per record and 32 per member more.
#include "sf_stream_core.h"

namespace sf {

namespace {

// members mode: the body bit behind the member head at body byte `byte`, if one stands there and its header ends before hi_bit
__device__ __forceinline__ uint64_t member_body_candidate(const StreamItem& I, uint64_t byte, uint64_t hi_bit) {
  const uint64_t at = I.b0 + byte;
  if (!members::head_candidate(I.src, at, I.src_n)) return kNoCandidate;
  uint32_t st;
  const uint64_t bit = 8 * (members::header_end(I.src, at, I.src_n, st) - I.b0);
  return bit < hi_bit ? bit : kNoCandidate;
}

// one wave per nominal chunk row of the call; the row's item is the last whose first row c0 is at or before it
template <bool MEMBERS>
__global__ __launch_bounds__(KF_THREADS) void k_stream_find(const StreamItem* __restrict__ items, uint32_t nitems, uint32_t nc,
                                                            uint64_t step_bits, uint64_t* __restrict__ cand) {
  __shared__ uint8_t s_lut[KF_THREADS][128];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x * (KF_THREADS / 64) + wave;
  if (r >= nc) return;
  uint32_t lo = 0, hi = nitems;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (items[mid].c0 <= r) lo = mid;
    else hi = mid;
  }
  const StreamItem& I = items[lo];
  const uint32_t c = r - I.c0;
  if (c == 0) {
    if (lane == 0) cand[r] = 0;
    return;
  }
  const uint64_t bits = 8 * I.body_n, lo_bit = (uint64_t)c * step_bits;
  const uint64_t hi_bit = lo_bit + step_bits < bits ? lo_bit + step_bits : bits;
  for (uint64_t at = lo_bit; at < hi_bit; at += 64) {
    const uint64_t p = at + lane;
    bool hit = false;
    if (p < hi_bit) {
      StreamReader rd;
      rd.open(I.src, I.src_n, I.b0, I.body_n, p & ~7ull);
      hit = stored_header_candidate(rd.br, (uint32_t)(p & 7), p >> 3, I.body_n) &&
            stored_run_follows(I.src + I.b0, I.body_n, (p >> 3) + 5 + stored_header_len(rd.br));
      if (!hit) {
        rd.br.drop((uint32_t)(p & 7));
        hit = dynamic_header_candidate(rd.br, s_lut[threadIdx.x]);
      }
    }
    const uint64_t b = __ballot(hit);
    if (b) {
      if (lane == 0) cand[r] = at + (uint64_t)(__ffsll((unsigned long long)b) - 1);
      return;
    }
    if (MEMBERS) {  // no block start in these 64 bits: a member head at one of their 8 bytes?
      const uint64_t v = (lane & 7) == 0 && p < hi_bit ? member_body_candidate(I, p >> 3, hi_bit) : kNoCandidate;
      const uint64_t mb = __ballot(v != kNoCandidate);
      if (mb) {
        const uint64_t first = __shfl(v, __ffsll((unsigned long long)mb) - 1);
        if (lane == 0) cand[r] = first;
        return;
      }
    }
  }
  if (lane == 0) cand[r] = kNoCandidate;
}

// list: the records to decode (nullable: 0..n-1; a repair round: the records to decode again), each against its item's stream,
// plane (write: plane + I.plane) and capacity.  follow (count pass; one lane per list entry: an item's first broken link behind
// its confirmed chain, already decoded again): the lane goes on into the records after it while their links break -- each next
// chunk starts where the one before ended, as the host's chain round would set it -- until a link holds or its item's records
// end, so a repair never runs into the next item.  A run of false candidates (stored blocks full of DEFLATE data put one in
// nearly every nominal chunk) is then mended in one round instead of one link per round; the other lanes' speculative repairs
// of the round have finished (an earlier launch), so no record is written by two lanes.
template <bool WRITE, bool MEMBERS>
__global__ __launch_bounds__(KS_LANES) void k_stream_decode(const StreamItem* __restrict__ items,
                                                            const uint32_t* __restrict__ rec_item, StreamChunk* __restrict__ recs,
                                                            const uint32_t* __restrict__ list, uint32_t n, bool follow,
                                                            uint16_t* __restrict__ plane, StreamSide* __restrict__ side,
                                                            StreamMember* __restrict__ mem) {
  extern __shared__ __align__(16) uint8_t s_tables[];
  const uint32_t k = blockIdx.x * KS_LANES + threadIdx.x;
  if (k >= n) return;
  uint8_t* tab = s_tables + threadIdx.x * LaneLayout::kBytes;
  if (WRITE && follow) return;
  uint32_t i = list ? list[k] : k;
  const StreamItem& I = items[rec_item[i]];
  const uint32_t m = I.r0 + I.m;
  for (uint32_t j = follow ? i + 1 : i; j < m; i = j++) {
    if (follow) {
      StreamChunk& a = recs[i];
      StreamChunk& b = recs[j];
      if (a.status != 0 || a.final_ || a.end == b.start) break;
      a.limit = a.end;  // (as stream_chain_round: the same decode)
      b.start = a.end;
    }
    if (MEMBERS)
      stream_decode<WRITE, true>(I.src, I.src_n, I.b0, I.body_n, recs[j], tab, WRITE ? plane + I.plane : plane, I.cap, side + j, mem,
                                 rec_item[j]);
    else
      stream_decode<WRITE, false>(I.src, I.src_n, I.b0, I.body_n, recs[j], tab, WRITE ? plane + I.plane : plane, I.cap);
    if (!follow) break;  // (follow: b.start >= b.limit is an empty chunk)
  }
}

// row (item, group), every group but an item's last: the composite map of the group's chunks over the window before its first
// chunk (group 0: the window itself, whose bytes before the stream are never read)
__global__ __launch_bounds__(KR_THREADS) void k_stream_compose(const uint16_t* __restrict__ plane,
                                                               const StreamChunk* __restrict__ recs,
                                                               const StreamItem* __restrict__ items,
                                                               const StreamGroup* __restrict__ rows,
                                                               uint16_t* __restrict__ tables) {
  __shared__ uint16_t T[kWin];
  const StreamGroup R = rows[blockIdx.x];
  const StreamItem& I = items[R.item];
  const uint32_t g = R.g, G = I.G, n = I.chain;
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) T[j] = g ? (uint16_t)(0x8000u | j) : 0;
  __syncthreads();
  const uint32_t i1 = (g + 1) * G < n ? (g + 1) * G : n;
  for (uint32_t i = g * G; i < i1; ++i) window_step(T, plane + I.plane, recs[I.r0 + i]);
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) tables[I.win + (size_t)g * kWin + j] = T[j];
}

// one workgroup per listed item (those of more than one group), all of them at once: the item's tables[g] <- the window after
// its group g, in bytes (tables[0] is that already)
__global__ __launch_bounds__(KR_THREADS) void k_stream_link(const StreamItem* __restrict__ items,
                                                            const uint32_t* __restrict__ link, uint16_t* __restrict__ tables) {
  __shared__ uint16_t W[kWin];
  const StreamItem& I = items[link[blockIdx.x]];
  const uint32_t ng = (I.chain + I.G - 1) / I.G;
  uint16_t* t = tables + I.win;
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) W[j] = t[j];
  __syncthreads();
  for (uint32_t g = 1; g + 1 < ng; ++g) {
    uint16_t v[kPerThread];
    uint16_t* C = t + (size_t)g * kWin;
#pragma unroll
    for (uint32_t r = 0; r < kPerThread; ++r) {
      const uint16_t x = C[r * KR_THREADS + threadIdx.x];
      v[r] = x < 256 ? x : W[x & 0x7FFFu];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kPerThread; ++r) {
      W[r * KR_THREADS + threadIdx.x] = v[r];
      C[r * KR_THREADS + threadIdx.x] = v[r];
    }
    __syncthreads();
  }
}

// row (item, group): the group's chunks' bytes into the item's dst, each from its window, then the window carried to the next
// chunk
__global__ __launch_bounds__(KR_THREADS) void k_stream_resolve(const uint16_t* __restrict__ plane,
                                                               const StreamChunk* __restrict__ recs,
                                                               const StreamItem* __restrict__ items,
                                                               const StreamGroup* __restrict__ rows,
                                                               const uint16_t* __restrict__ tables) {
  __shared__ uint16_t T[kWin];
  const StreamGroup R = rows[blockIdx.x];
  const StreamItem& I = items[R.item];
  const uint32_t g = R.g, G = I.G, n = I.chain;
  const uint16_t* p = plane + I.plane;
  uint8_t* dst = I.dst;
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) T[j] = g ? tables[I.win + (size_t)(g - 1) * kWin + j] : 0;
  __syncthreads();
  const uint32_t i1 = (g + 1) * G < n ? (g + 1) * G : n;
  for (uint32_t i = g * G; i < i1; ++i) {
    const StreamChunk c = recs[I.r0 + i];
    for (uint64_t q = threadIdx.x; q < c.out; q += KR_THREADS) {
      const uint16_t x = p[c.base + q];
      dst[c.base + q] = (uint8_t)(x < 256 ? x : T[x & 0x7FFFu]);
    }
    if (i + 1 < i1) window_step(T, p, c);
  }
}

}  // namespace

hipError_t launch_stream_find(const StreamItem* items, uint32_t nitems, uint32_t nc, uint64_t step_bytes, uint64_t* cand,
                              hipStream_t s, bool members) {
  if (nc == 0) return hipSuccess;
  const uint32_t per = KF_THREADS / 64;
  if (members)
    hipLaunchKernelGGL(k_stream_find<true>, dim3((nc + per - 1) / per), dim3(KF_THREADS), 0, s, items, nitems, nc, 8 * step_bytes, cand);
  else
    hipLaunchKernelGGL(k_stream_find<false>, dim3((nc + per - 1) / per), dim3(KF_THREADS), 0, s, items, nitems, nc, 8 * step_bytes, cand);
  return hipGetLastError();
}

hipError_t launch_stream_decode(bool write, const StreamItem* items, const uint32_t* rec_item, StreamChunk* recs,
                                const uint32_t* list, uint32_t n, bool follow, uint16_t* plane, hipStream_t s, StreamSide* side,
                                StreamMember* mem) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + KS_LANES - 1) / KS_LANES), block(KS_LANES);
  if (write && side)
    hipLaunchKernelGGL((k_stream_decode<true, true>), grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane, side, mem);
  else if (write)
    hipLaunchKernelGGL((k_stream_decode<true, false>), grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane, side, mem);
  else if (side)
    hipLaunchKernelGGL((k_stream_decode<false, true>), grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane, side, mem);
  else
    hipLaunchKernelGGL((k_stream_decode<false, false>), grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane, side, mem);
  return hipGetLastError();
}

uint32_t stream_group(uint32_t n) {
  uint32_t g = 1;
  while ((uint64_t)g * g < n) ++g;
  return g;
}

hipError_t launch_stream_resolve(const uint16_t* plane, const StreamChunk* recs, const StreamItem* items,
                                 const StreamGroup* compose, uint32_t ncompose, const uint32_t* link, uint32_t nlink,
                                 const StreamGroup* resolve, uint32_t nresolve, uint16_t* tables, hipStream_t s) {
  if (ncompose) {
    hipLaunchKernelGGL(k_stream_compose, dim3(ncompose), dim3(KR_THREADS), 0, s, plane, recs, items, compose, tables);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (nlink) {
    hipLaunchKernelGGL(k_stream_link, dim3(nlink), dim3(KR_THREADS), 0, s, items, link, tables);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (nresolve) hipLaunchKernelGGL(k_stream_resolve, dim3(nresolve), dim3(KR_THREADS), 0, s, plane, recs, items, resolve, tables);
  return hipGetLastError();
}

}  // namespace sf
