// sf_unindexed.hip -- the segment index of block-flushed DEFLATE streams, recovered from the streams alone, and
// the device pass the decoder needs on such an index.  One kernel set: the bodies of a call are scanned and walked together,
// and a single stream (sfh_recover_index*, sfh_decompress_any*) is a call of one item (sfh_recover_index_batch*,
// sfh_decompress_any_batch*).
//
//   k_any_scan<WRITE>  one pass over every body (a stream without its wrapper): every position p with [p-4, p) = 00 00 FF FF
//                      (M, the end of a flush) and every h with [h, h+5) = 00|01 00 80 FF 7F (H, the header of a stored block of
//                      32 KiB), plus the body's first byte b0.  One wave per 8 KiB of ONE item's stream; a wave-round with no
//                      hit costs one ballot.  WRITE = 0 counts the wave's nodes, WRITE = 1 writes them in stream order at the
//                      wave's offset (an exclusive scan of the counts): no atomics, the node list comes out sorted, item
//                      after item, each item's list closed by its end sentinel.
//   k_any_ranges       per item, its nodes and its M nodes in the concatenated lists.
//   k_any_succ         every node's successor on the walk (the walk rule), inside its item, and how many segments
//                      the edge covers.
//   k_any_jump         one round of pointer jumping that also spreads the mark "on the chain from b0": after round r every
//                      node at most 2^(r+1) - 1 steps behind its item's b0 is marked.  Nodes off the chain (flush markers and
//                      fake headers inside stored payloads) are never marked, and a run of stored segments costs no serial steps.
//   k_any_scatter      marked node of rank k in its item (an exclusive scan of the edge labels) -> the item's index[k] (and
//                      index[k+1] for the coded segment a stored jump lands on); at the sentinel, whether the chain holds the
//                      item's segments.  An item whose chain does not is written nowhere: its entries stay 0.
//   k_any_single       the items of one segment, which need no scan: index [b0, e].
//   k_any_depends      after the token stage: per segment of a launch batch, does a match reach before its first byte?
//   k_any_rows_*       strip rows for k_inflate_bytes: an independent segment and the dependent ones behind it.
#include "sf_device.h"

#include "sf_inflate_core.h"

namespace sf {

namespace {

constexpr uint32_t KA_THREADS = 256;
constexpr uint32_t KA_WAVE_BYTES = 8192;  // stream bytes per wave of k_any_scan (32 rounds of 64 lanes x 4 bytes)
constexpr uint32_t KA_ROUNDS = KA_WAVE_BYTES / 256;
constexpr uint8_t kNodeM = 1, kNodeH = 2;
constexpr uint32_t kStoredSeg = kChunk + 5;  // a stored segment: header byte, LEN, NLEN, 32 KiB

__device__ __forceinline__ uint32_t dword_at(const uint8_t* src, uint64_t src_n, int64_t k) {
  // dword k of the buffer (readable up to the next multiple of 4 bytes); zero outside it
  if (k < 0 || (uint64_t)k * 4 >= src_n) return 0u;
  return reinterpret_cast<const uint32_t*>(src)[k];
}

// the hits of the four positions 4k .. 4k+3: bits 0..3 M, 4..7 H, 8..11 the body's first byte
__device__ __forceinline__ uint32_t hits_at(const uint8_t* src, uint64_t src_n, uint64_t b0, uint64_t e, int64_t k) {
  const uint64_t prev = dword_at(src, src_n, k - 1), cur = dword_at(src, src_n, k), next = dword_at(src, src_n, k + 1);
  const uint64_t lo = (cur << 32) | prev, hi = (next << 32) | cur;
  uint32_t m = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint64_t p = 4 * (uint64_t)k + j;
    if (p < b0 || p >= e) continue;
    if (p >= b0 + 4 && (uint32_t)(lo >> (8 * j)) == 0xFFFF0000u) m |= 1u << j;
    const uint64_t h = hi >> (8 * j);
    if (p + 5 <= e && (h & 0xFEu) == 0 && (uint32_t)(h >> 8) == 0x7FFF8000u) m |= 16u << j;
    if (p == b0) m |= 256u << j;
  }
  return m;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// where the segment after a stored segment at p starts: behind its 32 KiB, and behind the empty stored blocks a flush writes
__device__ __forceinline__ uint64_t landing(const uint8_t* src, uint64_t p, uint64_t e) {
  uint64_t t = p + kStoredSeg;
  while (t + 5 <= e && src[t] == 0 && src[t + 1] == 0 && src[t + 2] == 0 && src[t + 3] == 0xFF && src[t + 4] == 0xFF) t += 5;
  return t;
}

// first node at or after position t (binary search over the sorted positions)
__device__ __forceinline__ uint32_t lower_bound(const uint64_t* pos, uint32_t n, uint64_t t) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pos[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- exclusive scan of uint32 (1024 per block, then the block sums in one workgroup, then the add) ----
constexpr uint32_t KS_T = 256, KS_PER = 4, KS_TILE = KS_T * KS_PER;
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v);
  if (lane == 63) s_w[w] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t k = 0; k < KS_T / 64; ++k) {
    before += k < w ? s_w[k] : 0u;
    total += s_w[k];
  }
  __syncthreads();
  return before + incl - v;
}
__global__ __launch_bounds__(KS_T) void k_scan_tiles(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n,
                                                     uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_w[KS_T / 64];
  const uint64_t base = (uint64_t)blockIdx.x * KS_TILE + threadIdx.x * KS_PER;
  uint32_t v[KS_PER], t = 0;
  for (uint32_t j = 0; j < KS_PER; ++j) {
    v[j] = base + j < n ? in[base + j] : 0u;
    t += v[j];
  }
  uint32_t total;
  uint32_t run = block_excl_scan(t, s_w, total);
  for (uint32_t j = 0; j < KS_PER; ++j) {
    if (base + j < n) out[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(KS_T) void k_scan_top(uint32_t* __restrict__ sums, uint32_t nt, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_w[KS_T / 64];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < nt; b += KS_T) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < nt ? sums[i] : 0u;
    uint32_t t;
    const uint32_t x = block_excl_scan(v, s_w, t);
    if (i < nt) sums[i] = carry + x;
    carry += t;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(KS_T) void k_scan_add(uint32_t* __restrict__ out, uint32_t n, const uint32_t* __restrict__ sums) {
  const uint64_t base = (uint64_t)blockIdx.x * KS_TILE + threadIdx.x * KS_PER;
  const uint32_t add = sums[blockIdx.x];
  for (uint32_t j = 0; j < KS_PER; ++j)
    if (base + j < n) out[base + j] += add;
}

// ---- the bodies of a call ----
// The node list is the items' lists one after the other, each closed by its own end sentinel (kNodeS, at the body's end e: the
// last wave of an item writes it); item[at] names a node's item, range[item] its nodes [n0, n1) (n1: the sentinel) and its M
// nodes [m0, m1) in the concatenated lists.  An item of one segment has no waves and no nodes (k_any_single).
constexpr uint8_t kNodeS = 4;

// one wave per 8 KiB of ONE item's stream (waves[wave] = {item, piece}): hits are tested against the item's own base and body,
// so a pattern is never seen across two items that lie back to back
template <bool WRITE>
__global__ __launch_bounds__(KA_THREADS) void k_any_scan(const AnyItem* __restrict__ items, const AnyWave* __restrict__ waves,
                                                         const uint64_t* __restrict__ heads, uint32_t nwaves,
                                                         uint32_t* __restrict__ cnt_nodes, uint32_t* __restrict__ cnt_m,
                                                         uint64_t* __restrict__ pos, uint8_t* __restrict__ flg,
                                                         uint32_t* __restrict__ minc, uint32_t* __restrict__ midx,
                                                         uint32_t* __restrict__ item) {
  const uint32_t wave = blockIdx.x * (KA_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wave >= nwaves) return;
  const AnyWave W = waves[wave];
  const AnyItem I = items[W.item];
  const uint8_t* src = row_ptr(I.src);  // (global loads, as with the stream a kernel argument)
  const uint64_t src_n = I.src_n, b0 = heads[2 * (size_t)W.item], e = heads[2 * (size_t)W.item + 1];
  uint32_t nodes = WRITE ? cnt_nodes[wave] : 0u, ms = WRITE ? cnt_m[wave] : 0u;
  const int64_t k0 = (int64_t)W.piece * (KA_WAVE_BYTES / 4);
  for (uint32_t r = 0; r < KA_ROUNDS; ++r) {
    const int64_t k = k0 + r * 64 + lane;
    const uint32_t h = hits_at(src, src_n, b0, e, k);
    if (__ballot(h != 0) == 0) continue;
    const uint32_t pm = h & 15u, any = (h | (h >> 4) | (h >> 8)) & 15u;
    const uint32_t n_incl = wave_incl_scan(__popc(any)), m_incl = wave_incl_scan(__popc(pm));
    if constexpr (WRITE) {
      uint32_t at = nodes + n_incl - __popc(any), mat = ms + m_incl - __popc(pm);
      for (uint32_t j = 0; j < 4; ++j) {
        if (!((any >> j) & 1u)) continue;
        const bool is_m = (pm >> j) & 1u;
        pos[at] = 4 * (uint64_t)k + j;
        flg[at] = (is_m ? kNodeM : 0) | (((h >> (4 + j)) & 1u) ? kNodeH : 0);
        item[at] = W.item;
        if (is_m) midx[mat++] = at;
        minc[at] = mat;  // M nodes (of the call) at or before this one
        ++at;
      }
    }
    nodes += (uint32_t)__shfl((int)n_incl, 63, 64);
    ms += (uint32_t)__shfl((int)m_incl, 63, 64);
  }
  const bool last = W.piece + 1 == I.nwaves;  // the item's sentinel stands behind its last node
  if (lane == 0) {
    if constexpr (WRITE) {
      if (last) {
        pos[nodes] = e;
        flg[nodes] = kNodeS;
        item[nodes] = W.item;
        minc[nodes] = ms;
      }
    } else {
      cnt_nodes[wave] = nodes + (last ? 1u : 0u);
      cnt_m[wave] = ms;
    }
  }
}

// per item, from the scanned counts: its node and M ranges; tot[5]: the largest item's nodes (the rounds of the jump)
__global__ __launch_bounds__(KA_THREADS) void k_any_ranges(const AnyItem* __restrict__ items, uint32_t nitems,
                                                           const uint32_t* __restrict__ node_off, const uint32_t* __restrict__ m_off,
                                                           uint32_t nwaves, const uint32_t* __restrict__ tot,
                                                           AnyRange* __restrict__ range, uint32_t* __restrict__ largest) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i >= nitems) return;
  const AnyItem I = items[i];
  AnyRange R{0, 0, 0, 0};
  if (I.nwaves) {
    const uint32_t w1 = I.wave0 + I.nwaves;
    R.n0 = node_off[I.wave0];
    R.n1 = (w1 < nwaves ? node_off[w1] : tot[0]) - 1;
    R.m0 = m_off[I.wave0];
    R.m1 = w1 < nwaves ? m_off[w1] : tot[1];
    atomicMax(largest, R.n1 - R.n0);
  }
  range[i] = R;
}

// The walk rule: from a start s in H the next start is landing(s); from any other start, the first M after s.  A landing
// that is no node is a coded segment's start whose own successor is the first M after it: that edge covers two segments.
// Over the concatenated list: the search and the M lists are confined to the node's item, its sentinel is a self-loop and the
// mark starts at the item's first node.
__global__ __launch_bounds__(KA_THREADS) void k_any_succ(const AnyItem* __restrict__ items, const uint64_t* __restrict__ heads,
                                                         const AnyRange* __restrict__ range, const uint32_t* __restrict__ item,
                                                         const uint64_t* __restrict__ pos, const uint8_t* __restrict__ flg,
                                                         const uint32_t* __restrict__ minc, const uint32_t* __restrict__ midx,
                                                         uint32_t ntot, uint32_t* __restrict__ nxt, uint8_t* __restrict__ lab,
                                                         uint8_t* __restrict__ mark) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i >= ntot) return;
  const uint32_t it = item[i];
  const AnyRange R = range[it];
  if (i == R.n1) {
    nxt[i] = i;  // the end of this item's body
    lab[i] = 0;
    mark[i] = 0;
    return;
  }
  const uint8_t* src = items[it].src;
  const uint64_t e = heads[2 * (size_t)it + 1];
  const uint64_t* ipos = pos + R.n0;
  const uint32_t n = R.n1 - R.n0;
  uint32_t s = R.n1, l = 1;
  if (flg[i] & kNodeH) {
    const uint64_t t = landing(src, pos[i], e);
    if (t < e) {
      const uint32_t j = lower_bound(ipos, n, t);
      if (j < n && ipos[j] == t) {
        s = R.n0 + j;
      } else {
        const uint32_t mi = j < n ? minc[R.n0 + j] - (flg[R.n0 + j] & kNodeM) : R.m1;  // M nodes before j
        s = mi < R.m1 ? midx[mi] : R.n1;
        l = 2;
      }
    }
  } else {
    const uint32_t mi = minc[i];
    s = mi < R.m1 ? midx[mi] : R.n1;
  }
  nxt[i] = s;
  lab[i] = (uint8_t)l;
  mark[i] = i == R.n0;
}

__global__ __launch_bounds__(KA_THREADS) void k_any_jump(const uint32_t* __restrict__ nxt, uint32_t* __restrict__ nxt2,
                                                         uint8_t* mark, uint32_t n) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i > n) return;
  const uint32_t j = nxt[i];
  // (a node marked by another lane of this round is on the chain as well: marks only ever spread along it)
  if (i < n && j < n && mark[i]) mark[j] = 1;
  nxt2[i] = nxt[j];
}

__global__ __launch_bounds__(KA_THREADS) void k_any_labels(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ mark,
                                                           uint32_t n, uint32_t* __restrict__ c) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i < n) c[i] = mark[i] ? lab[i] : 0u;
}

// rank: the exclusive scan of the labels over the whole list; a node's segment is its rank minus the rank of its item's first
// node, and the rank at the sentinel closes the item's chain total: ok[item] = the chain holds the item's nseg segments.
// index: flat, every item's nseg + 1 entries from its ix0 (sfh_copy_batch_index's layout)
__global__ __launch_bounds__(KA_THREADS) void k_any_scatter(const AnyItem* __restrict__ items, const uint64_t* __restrict__ heads,
                                                            const AnyRange* __restrict__ range, const uint32_t* __restrict__ item,
                                                            const uint64_t* __restrict__ pos, const uint8_t* __restrict__ lab,
                                                            const uint8_t* __restrict__ mark, const uint32_t* __restrict__ rank,
                                                            uint32_t ntot, uint64_t* __restrict__ index, uint32_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i >= ntot) return;
  const uint32_t it = item[i];
  const AnyRange R = range[it];
  const AnyItem I = items[it];
  const uint64_t e = heads[2 * (size_t)it + 1];
  uint64_t* ix = index + I.ix0;
  const uint32_t k = rank[i] - rank[R.n0];
  const bool holds = rank[R.n1] - rank[R.n0] >= I.nseg;  // (an item whose chain is too short keeps its zeroed entries)
  if (i == R.n1) {
    if (holds) ix[I.nseg] = e;
    ok[it] = holds ? 1u : 0u;
    return;
  }
  if (!mark[i] || !holds) return;
  if (k < I.nseg) ix[k] = pos[i];
  if (lab[i] == 2 && k + 1 < I.nseg) ix[k + 1] = landing(I.src, pos[i], e);
}

// the items of one segment: index [b0, e], indexable (an empty body included: the decoder says what is wrong with it)
__global__ __launch_bounds__(KA_THREADS) void k_any_single(const AnyItem* __restrict__ items, uint32_t nitems,
                                                           const uint64_t* __restrict__ heads, uint64_t* __restrict__ index,
                                                           uint32_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * KA_THREADS + threadIdx.x;
  if (i >= nitems || items[i].nwaves) return;
  index[items[i].ix0] = heads[2 * (size_t)i];
  index[items[i].ix0 + 1] = heads[2 * (size_t)i + 1];
  ok[i] = 1;
}

// ---- behind the token stage ----

// one wave per segment of a launch batch's segment table: 1 when a match of it reaches before its first byte (an item's first
// segment, which has no history and always starts a row, and failed or stored segments: 0)
__global__ __launch_bounds__(64) void k_any_depends(const InflateSeg* __restrict__ rows, const SegInfo* __restrict__ info,
                                                    const uint32_t* __restrict__ tokens, uint8_t* __restrict__ depends,
                                                    uint32_t* __restrict__ starts) {
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  const SegInfo I = info[seg];
  const bool first = (rows[seg].hist & ~(kSegWrapped | kSegExact)) == 0;
  bool dep = false;
  if (!first && I.status == inflate::kOk && !(I.raw & kSegRaw)) {
    const uint32_t* tk = tokens + (uint64_t)seg * kChunk;
    uint32_t out = 0;
    for (uint32_t t0 = 0; t0 < I.ntok && !dep; t0 += 64) {
      const uint32_t t = t0 + lane;
      uint32_t len = 0, dist = 0;
      if (t < I.ntok) {
        const uint32_t tok = tk[t];
        const bool m = (tok & inflate::kTokMatchBit) != 0;
        len = m ? ((tok >> 16) & 0x7FFFu) + 3u : 1u;
        dist = m ? (tok & 0xFFFFu) + 1u : 0u;
      }
      const uint32_t incl = wave_incl_scan(len);
      dep = __ballot(dist > out + incl - len) != 0;  // (a literal has dist 0)
      out += (uint32_t)__shfl((int)incl, 63, 64);
    }
  }
  if (lane == 0) {
    depends[seg] = dep ? 1 : 0;
    starts[seg] = dep ? 0u : 1u;
  }
}

// rows: row r starts at the r-th independent segment; slots past the last row are {0, 0} (the byte kernel's grid is nseg)
__global__ __launch_bounds__(KA_THREADS) void k_any_rows_a(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ excl,
                                                           const uint32_t* __restrict__ nrows, uint32_t nseg,
                                                           InflateStrip* __restrict__ rows) {
  const uint32_t k = blockIdx.x * KA_THREADS + threadIdx.x;
  if (k >= nseg) return;
  if (k >= *nrows) rows[k] = InflateStrip{0, 0};
  if (starts[k]) rows[excl[k]].seg0 = k;
}
__global__ __launch_bounds__(KA_THREADS) void k_any_rows_b(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ excl,
                                                           uint32_t nseg, InflateStrip* __restrict__ rows) {
  const uint32_t k = blockIdx.x * KA_THREADS + threadIdx.x;
  if (k >= nseg || !(k + 1 == nseg || starts[k + 1])) return;
  const uint32_t r = excl[k] + starts[k] - 1;  // the row segment k belongs to
  rows[r].nseg = k + 1 - rows[r].seg0;
}

inline uint32_t grid(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

uint32_t any_scan_waves(uint64_t src_n) { return (uint32_t)((src_n + KA_WAVE_BYTES - 1) / KA_WAVE_BYTES); }
size_t any_scan_tmp_words(uint32_t n) { return grid(n, KS_TILE) + 1; }

hipError_t launch_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tmp, uint32_t* total, hipStream_t s) {
  const uint32_t nt = grid(n, KS_TILE);
  if (nt) hipLaunchKernelGGL(k_scan_tiles, dim3(nt), dim3(KS_T), 0, s, in, out, n, tmp);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(KS_T), 0, s, tmp, nt, total);
  if (nt) hipLaunchKernelGGL(k_scan_add, dim3(nt), dim3(KS_T), 0, s, out, n, tmp);
  return hipGetLastError();
}

hipError_t launch_any_count(const AnyItem* items, const AnyWave* waves, const uint64_t* heads, uint32_t nwaves,
                            uint32_t* cnt_nodes, uint32_t* cnt_m, hipStream_t s) {
  hipLaunchKernelGGL(k_any_scan<false>, dim3(grid(nwaves, KA_THREADS / 64)), dim3(KA_THREADS), 0, s, items, waves, heads, nwaves,
                     cnt_nodes, cnt_m, (uint64_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                     (uint32_t*)nullptr);
  return hipGetLastError();
}

hipError_t launch_any_ranges(const AnyItem* items, uint32_t nitems, const uint32_t* node_off, const uint32_t* m_off, uint32_t nwaves,
                             const uint32_t* tot, AnyRange* range, uint32_t* largest, hipStream_t s) {
  hipLaunchKernelGGL(k_any_ranges, dim3(grid(nitems, KA_THREADS)), dim3(KA_THREADS), 0, s, items, nitems, node_off, m_off, nwaves, tot,
                     range, largest);
  return hipGetLastError();
}

hipError_t launch_any_nodes(const AnyItem* items, const AnyWave* waves, const uint64_t* heads, uint32_t nwaves,
                            uint32_t* node_off, uint32_t* m_off, uint64_t* pos, uint8_t* flg, uint32_t* minc, uint32_t* midx,
                            uint32_t* item, hipStream_t s) {
  hipLaunchKernelGGL(k_any_scan<true>, dim3(grid(nwaves, KA_THREADS / 64)), dim3(KA_THREADS), 0, s, items, waves, heads, nwaves,
                     node_off, m_off, pos, flg, minc, midx, item);
  return hipGetLastError();
}

hipError_t launch_any_walk(const AnyItem* items, const uint64_t* heads, const AnyRange* range, const uint32_t* item,
                           const uint64_t* pos, const uint8_t* flg, const uint32_t* minc, const uint32_t* midx, uint32_t ntot,
                           uint32_t largest, uint32_t* nxt_a, uint32_t* nxt_b, uint8_t* lab, uint8_t* mark, uint32_t* lbl,
                           uint32_t* rank, uint32_t* tmp, uint32_t* total, uint64_t* index, uint32_t* ok, hipStream_t s) {
  hipLaunchKernelGGL(k_any_succ, dim3(grid(ntot, KA_THREADS)), dim3(KA_THREADS), 0, s, items, heads, range, item, pos, flg, minc,
                     midx, ntot, nxt_a, lab, mark);
  // after round r the nodes up to 2^(r+1) - 1 steps behind an item's b0 are marked; a chain has at most `largest` nodes
  // (the list's last node is a sentinel: k_any_jump's n.  A sentinel it marks carries the label 0.)
  for (uint64_t reach = 1; reach < largest; reach <<= 1) {
    hipLaunchKernelGGL(k_any_jump, dim3(grid(ntot, KA_THREADS)), dim3(KA_THREADS), 0, s, nxt_a, nxt_b, mark, ntot - 1);
    std::swap(nxt_a, nxt_b);
  }
  hipLaunchKernelGGL(k_any_labels, dim3(grid(ntot, KA_THREADS)), dim3(KA_THREADS), 0, s, lab, mark, ntot, lbl);
  hipError_t e = launch_scan_u32(lbl, rank, ntot, tmp, total, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_any_scatter, dim3(grid(ntot, KA_THREADS)), dim3(KA_THREADS), 0, s, items, heads, range, item, pos, lab,
                     mark, rank, ntot, index, ok);
  return hipGetLastError();
}

hipError_t launch_any_single(const AnyItem* items, uint32_t nitems, const uint64_t* heads, uint64_t* index, uint32_t* ok,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_any_single, dim3(grid(nitems, KA_THREADS)), dim3(KA_THREADS), 0, s, items, nitems, heads, index, ok);
  return hipGetLastError();
}

hipError_t launch_any_rows(const InflateSeg* segs, const SegInfo* info, const uint32_t* tokens, uint32_t nseg, uint8_t* depends,
                           uint32_t* starts, uint32_t* excl, uint32_t* tmp, uint32_t* nrows, InflateStrip* rows,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_any_depends, dim3(nseg), dim3(64), 0, s, segs, info, tokens, depends, starts);
  hipError_t e = launch_scan_u32(starts, excl, nseg, tmp, nrows, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_any_rows_a, dim3(grid(nseg, KA_THREADS)), dim3(KA_THREADS), 0, s, starts, excl, nrows, nseg, rows);
  hipLaunchKernelGGL(k_any_rows_b, dim3(grid(nseg, KA_THREADS)), dim3(KA_THREADS), 0, s, starts, excl, nseg, rows);
  return hipGetLastError();
}

}  // namespace sf
