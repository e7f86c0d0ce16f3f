// sf_stream_batch.hip -- many raw, zlib or gzip streams without flush points decoded in one call (sfh_inflate_stream_batch*,
// DESIGN.md 3a "Batches of streams without flush points").  The passes of sf_stream.hip, each kernel reading its item's stream,
// body, plane, capacity and output from a StreamItem row (sf_device.h) and calling the same device functions
// (sf_stream_core.h):
//
//   k_stream_find_batch        A. one wave per nominal chunk of the call; an item's local chunk 0 starts at its body's bit 0
//   k_stream_decode_batch<0>   B, C. one lane per record (a record's item: rec_item); a follow lane per item with a broken link
//                                 stops at its item's last record, so a repair never runs into the next item
//   k_stream_decode_batch<1>   D. the confirmed records of a launch batch's items, into plane + the item's offset: a record's
//                                 base stays item-relative, so the distance and capacity checks are the single call's
//   k_stream_compose_batch     F. rows of (item, group), groups of stream_group(chain) chunks per item; link: one workgroup
//   k_stream_link_batch           per item of more than one group, all of them at once; resolve writes into the item's dst
//   k_stream_resolve_batch
#include "sf_stream_core.h"

namespace sf {

namespace {

// as k_stream_decode: each lane decodes its record against its item's stream, plane (write: plane + I.plane, so a record's
// base stays item-relative) and capacity.  follow: one lane per item with a broken link, which stops at its item's last record.
template <bool WRITE>
__global__ __launch_bounds__(KS_LANES) void k_stream_decode_batch(const StreamItem* __restrict__ items,
                                                                  const uint32_t* __restrict__ rec_item,
                                                                  StreamChunk* __restrict__ recs, const uint32_t* __restrict__ list,
                                                                  uint32_t n, bool follow, uint16_t* __restrict__ plane) {
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
    stream_decode<WRITE>(I.src, I.src_n, I.b0, I.body_n, recs[j], tab, WRITE ? plane + I.plane : plane, I.cap);
    if (!follow) break;
  }
}

// one wave per nominal chunk row of the call; the row's item is the last whose first row c0 is at or before it
__global__ __launch_bounds__(KF_THREADS) void k_stream_find_batch(const StreamItem* __restrict__ items, uint32_t nitems,
                                                                  uint32_t nc, uint64_t step_bits, uint64_t* __restrict__ cand) {
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
      rd.open(I.src, I.src_n, I.b0, I.body_n, p);
      hit = dynamic_header_candidate(rd.br, s_lut[threadIdx.x]);
    }
    const uint64_t b = __ballot(hit);
    if (b) {
      if (lane == 0) cand[r] = at + (uint64_t)(__ffsll((unsigned long long)b) - 1);
      return;
    }
  }
  if (lane == 0) cand[r] = kNoCandidate;
}

// as k_stream_compose, for the row's (item, group)
__global__ __launch_bounds__(KR_THREADS) void k_stream_compose_batch(const uint16_t* __restrict__ plane,
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

// as k_stream_link: one workgroup per listed item, all of them at once
__global__ __launch_bounds__(KR_THREADS) void k_stream_link_batch(const StreamItem* __restrict__ items,
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

// as k_stream_resolve, for the row's (item, group), into the item's dst
__global__ __launch_bounds__(KR_THREADS) void k_stream_resolve_batch(const uint16_t* __restrict__ plane,
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

hipError_t launch_stream_find_batch(const StreamItem* items, uint32_t nitems, uint32_t nc, uint64_t step_bytes, uint64_t* cand,
                                    hipStream_t s) {
  if (nc == 0) return hipSuccess;
  const uint32_t per = KF_THREADS / 64;
  hipLaunchKernelGGL(k_stream_find_batch, dim3((nc + per - 1) / per), dim3(KF_THREADS), 0, s, items, nitems, nc, 8 * step_bytes, cand);
  return hipGetLastError();
}

hipError_t launch_stream_decode_batch(bool write, const StreamItem* items, const uint32_t* rec_item, StreamChunk* recs,
                                      const uint32_t* list, uint32_t n, bool follow, uint16_t* plane, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + KS_LANES - 1) / KS_LANES), block(KS_LANES);
  if (write)
    hipLaunchKernelGGL(k_stream_decode_batch<true>, grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane);
  else
    hipLaunchKernelGGL(k_stream_decode_batch<false>, grid, block, KS_LDS, s, items, rec_item, recs, list, n, follow, plane);
  return hipGetLastError();
}

hipError_t launch_stream_resolve_batch(const uint16_t* plane, const StreamChunk* recs, const StreamItem* items,
                                       const StreamGroup* compose, uint32_t ncompose, const uint32_t* link, uint32_t nlink,
                                       const StreamGroup* resolve, uint32_t nresolve, uint16_t* tables, hipStream_t s) {
  if (ncompose) {
    hipLaunchKernelGGL(k_stream_compose_batch, dim3(ncompose), dim3(KR_THREADS), 0, s, plane, recs, items, compose, tables);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (nlink) {
    hipLaunchKernelGGL(k_stream_link_batch, dim3(nlink), dim3(KR_THREADS), 0, s, items, link, tables);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (nresolve) hipLaunchKernelGGL(k_stream_resolve_batch, dim3(nresolve), dim3(KR_THREADS), 0, s, plane, recs, items, resolve, tables);
  return hipGetLastError();
}


}  // namespace sf
