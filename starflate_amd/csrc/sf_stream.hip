// sf_stream.hip -- one raw, zlib or gzip stream (one member) decoded on the GPU with no side information and no flush points
// (sfh_inflate_stream*, DESIGN.md 3a "Streams without flush points").  The body (the stream without its wrapper) is cut into
// chunks at speculative block starts, the chunks are decoded lane-serially, and a chain rule keeps exactly the serial decoder's
// block sequence:
//
//   k_stream_find        A. one wave per nominal chunk start (every S body bytes, S = SFH_STREAM_CHUNK): the first bit offset
//                           before the next nominal start where dynamic_header_candidate (sf_inflate_core.h) holds.  Chunk 0
//                           starts at the body's first bit whatever its block type.
//   k_stream_decode<0>   B. one lane per chunk: whole blocks from the chunk's start until the first block end at or beyond the
//                           next chunk's start (the last chunk: until BFINAL or an error).  Records the end bit, the output
//                           bytes, BFINAL and the first structural problem.  The checks that need the absolute output position
//                           (distance <= bytes written, dst capacity) wait for the write pass.
//                        C. on the host (sf_stream_chain.h): chunk i+1 is confirmed when chunk i is and ended, without BFINAL,
//                           exactly on i+1's start.  Every broken link is redecoded from the end before it, all of a round in
//                           parallel; then one lane follows the first of them through the run of broken links behind it.
//   k_stream_decode<1>   D. the confirmed chain again, with the exact rules now that each chunk's output offset O_i (an
//                           exclusive scan of the counts) and the capacity are known.  Every output byte becomes a u16 in the
//                           symbol plane: a literal byte (< 256), or 0x8000 | k, byte k of the 32 KiB window before O_i.
//   k_stream_compose     F. the window of chunk i+1 is a map of chunk i's tail over chunk i's window.  Groups of G ~ sqrt(N)
//   k_stream_link           chunks compose their maps in parallel (compose), one workgroup carries the window across the
//   k_stream_resolve        groups (link, N/G steps), and every group then writes its chunks' final bytes (resolve).
//
// The statuses are the serial decoder's (include/starflate/decompress.hpp): stream_decode follows its checks in its order,
// including where the input runs out.  A stream with no candidates (Z_FIXED, level 0, ...) is decoded by one lane: slow, but
// correct.  Bit positions and output counts are 64-bit; the 32-bit BitReader is re-opened before its position passes 2^30.
// Scratch: 2 bytes per output byte (the plane), 64 KiB per group, 60 bytes per nominal chunk.
#include "sf_stream_core.h"

namespace sf {

namespace {

using namespace inflate;

__global__ __launch_bounds__(KF_THREADS) void k_stream_find(const uint8_t* __restrict__ src, uint64_t src_n, uint64_t b0,
                                                            uint64_t body_n, uint64_t step_bits, uint32_t nc,
                                                            uint64_t* __restrict__ cand) {
  __shared__ uint8_t s_lut[KF_THREADS][128];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t c = blockIdx.x * (KF_THREADS / 64) + wave;
  if (c >= nc) return;
  if (c == 0) {
    if (lane == 0) cand[0] = 0;
    return;
  }
  const uint64_t bits = 8 * body_n, lo = (uint64_t)c * step_bits;
  const uint64_t hi = lo + step_bits < bits ? lo + step_bits : bits;
  for (uint64_t at = lo; at < hi; at += 64) {
    const uint64_t p = at + lane;
    bool hit = false;
    if (p < hi) {
      StreamReader rd;
      rd.open(src, src_n, b0, body_n, p);
      hit = dynamic_header_candidate(rd.br, s_lut[threadIdx.x]);
    }
    const uint64_t b = __ballot(hit);
    if (b) {
      if (lane == 0) cand[c] = at + (uint64_t)(__ffsll((unsigned long long)b) - 1);
      return;
    }
  }
  if (lane == 0) cand[c] = kNoCandidate;
}

// list: the records to decode (a repair round: the chunks to decode again).  follow (count pass; one lane, list[0]: the first
// broken link behind the confirmed chain, already decoded again): the lane goes on into the chunks after it while their links
// break -- each next chunk starts where the one before ended, as the host's chain round would set it -- until a link holds or
// the records end.  A run of false candidates (stored blocks full of DEFLATE data put one in nearly every nominal chunk) is
// then mended in one round instead of one link per round; the other lanes' speculative repairs of the round have finished (an
// earlier launch), so no record is written by two lanes.
template <bool WRITE>
__global__ __launch_bounds__(KS_LANES) void k_stream_decode(const uint8_t* __restrict__ src, uint64_t src_n, uint64_t b0,
                                                            uint64_t body_n, StreamChunk* __restrict__ recs,
                                                            const uint32_t* __restrict__ list, uint32_t n, uint32_t m,
                                                            bool follow, uint16_t* __restrict__ plane, uint64_t cap) {
  extern __shared__ __align__(16) uint8_t s_tables[];
  const uint32_t k = blockIdx.x * KS_LANES + threadIdx.x;
  if (k >= n) return;
  uint8_t* tab = s_tables + threadIdx.x * LaneLayout::kBytes;
  uint32_t i = list ? list[k] : k;
  if (!follow) {
    stream_decode<WRITE>(src, src_n, b0, body_n, recs[i], tab, plane, cap);
    return;
  }
  if (WRITE || k != 0) return;
  for (uint32_t j = i + 1; j < m; i = j++) {
    StreamChunk& a = recs[i];
    StreamChunk& b = recs[j];
    if (a.status != 0 || a.final_ || a.end == b.start) break;
    a.limit = a.end;  // (as stream_chain_round: the same decode)
    b.start = a.end;
    stream_decode<false>(src, src_n, b0, body_n, b, tab, plane, cap);  // (b.start >= b.limit: an empty chunk)
  }
}

// group g (all but the last): the composite map of its chunks over the window before its first chunk (group 0: the window
// itself, whose bytes before the stream are never read)
__global__ __launch_bounds__(KR_THREADS) void k_stream_compose(const uint16_t* __restrict__ plane,
                                                               const StreamChunk* __restrict__ recs, uint32_t n, uint32_t G,
                                                               uint16_t* __restrict__ tables) {
  __shared__ uint16_t T[kWin];
  const uint32_t g = blockIdx.x;
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) T[j] = g ? (uint16_t)(0x8000u | j) : 0;
  __syncthreads();
  const uint32_t i1 = (g + 1) * G < n ? (g + 1) * G : n;
  for (uint32_t i = g * G; i < i1; ++i) window_step(T, plane, recs[i]);
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) tables[(size_t)g * kWin + j] = T[j];
}

// one workgroup: tables[g] <- the window after group g, in bytes (tables[0] is that already)
__global__ __launch_bounds__(KR_THREADS) void k_stream_link(uint16_t* __restrict__ tables, uint32_t ng) {
  __shared__ uint16_t W[kWin];
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) W[j] = tables[j];
  __syncthreads();
  for (uint32_t g = 1; g + 1 < ng; ++g) {
    uint16_t v[kPerThread];
    uint16_t* C = tables + (size_t)g * kWin;
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

// group g: its chunks' bytes into dst, each from its window, then the window carried to the next chunk
__global__ __launch_bounds__(KR_THREADS) void k_stream_resolve(const uint16_t* __restrict__ plane,
                                                               const StreamChunk* __restrict__ recs, uint32_t n, uint32_t G,
                                                               const uint16_t* __restrict__ tables, uint8_t* __restrict__ dst) {
  __shared__ uint16_t T[kWin];
  const uint32_t g = blockIdx.x;
  for (uint32_t j = threadIdx.x; j < kWin; j += KR_THREADS) T[j] = g ? tables[(size_t)(g - 1) * kWin + j] : 0;
  __syncthreads();
  const uint32_t i1 = (g + 1) * G < n ? (g + 1) * G : n;
  for (uint32_t i = g * G; i < i1; ++i) {
    const StreamChunk c = recs[i];
    for (uint64_t p = threadIdx.x; p < c.out; p += KR_THREADS) {
      const uint16_t x = plane[c.base + p];
      dst[c.base + p] = (uint8_t)(x < 256 ? x : T[x & 0x7FFFu]);
    }
    if (i + 1 < i1) window_step(T, plane, c);
  }
}

}  // namespace

hipError_t launch_stream_find(const uint8_t* src, uint64_t src_n, uint64_t b0, uint64_t body_n, uint64_t step_bytes, uint32_t nc,
                              uint64_t* cand, hipStream_t s) {
  const uint32_t per = KF_THREADS / 64;
  hipLaunchKernelGGL(k_stream_find, dim3((nc + per - 1) / per), dim3(KF_THREADS), 0, s, src, src_n, b0, body_n, 8 * step_bytes,
                     nc, cand);
  return hipGetLastError();
}

hipError_t launch_stream_decode(bool write, const uint8_t* src, uint64_t src_n, uint64_t b0, uint64_t body_n, StreamChunk* recs,
                                const uint32_t* list, uint32_t n, uint32_t m, bool follow, uint16_t* plane, uint64_t cap,
                                hipStream_t s) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + KS_LANES - 1) / KS_LANES), block(KS_LANES);
  if (write)
    hipLaunchKernelGGL(k_stream_decode<true>, grid, block, KS_LDS, s, src, src_n, b0, body_n, recs, list, n, m, follow, plane, cap);
  else
    hipLaunchKernelGGL(k_stream_decode<false>, grid, block, KS_LDS, s, src, src_n, b0, body_n, recs, list, n, m, follow, plane, cap);
  return hipGetLastError();
}

uint32_t stream_group(uint32_t n) {
  uint32_t g = 1;
  while ((uint64_t)g * g < n) ++g;
  return g;
}

hipError_t launch_stream_resolve(const uint16_t* plane, const StreamChunk* recs, uint32_t n, uint16_t* tables, uint8_t* dst,
                                 hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t G = stream_group(n), ng = (n + G - 1) / G;
  if (ng > 1) {
    hipLaunchKernelGGL(k_stream_compose, dim3(ng - 1), dim3(KR_THREADS), 0, s, plane, recs, n, G, tables);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_stream_link, dim3(1), dim3(KR_THREADS), 0, s, tables, ng);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_stream_resolve, dim3(ng), dim3(KR_THREADS), 0, s, plane, recs, n, G, tables, dst);
  return hipGetLastError();
}

}  // namespace sf
