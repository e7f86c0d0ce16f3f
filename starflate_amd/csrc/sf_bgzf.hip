// sf_bgzf.hip -- the members of a BGZF file found on the device (sfh_bgzf_read_index_device; the format and the parser:
// sf_bgzf_plan.h).  Every member states its own length, so the file is a linked list from byte 0 -- and a list is walked in
// parallel the way DESIGN.md 3a recovers flush points:
//   k_bgzf_scan     every byte position that parses as a member's head is a NODE (256 lanes x 32 positions per workgroup; a
//                   position is parsed only where its first four bytes have the head's shape).  Run twice: the count per
//                   workgroup, then -- behind an exclusive scan of the counts -- the nodes themselves, ascending by position
//   k_bgzf_succ     a node's successor is the node at its position + BSIZE + 1 (a binary search over the positions); none:
//                   the sentinel behind the last node
//   k_bgzf_jump     pointer jumping, log2(nodes) rounds: every node's hops to the sentinel, and -- marks pushed along the
//                   same jumps -- the nodes the chain from position 0 reaches.  A head-shaped pattern inside compressed
//                   data is a node nobody reaches: it is never marked and changes nothing
//   k_bgzf_end      the reached node next to the sentinel: the chain ends at the file's end, or the status of the member
//                   that fails to parse there (no node at 0: of the member at 0)
//   k_bgzf_scatter  reached nodes in order (rank = hops of node 0 - own hops): member_off, and the ISIZEs by rank
//   k_bgzf_finish   one workgroup: the prefix sums of ISIZE (64-bit), the largest ISIZE, the EOF member, the info
// All reads of the file are parse_member's, bounded by src_n, and the scan's aligned dwords below it.
// Random access (sfh_decompress_bgzf_ranges*; the planner: sf_bgzf_range_plan.h), from the index the walk left on the device:
//   k_bgzf_range_spans  one lane per range: the two binary searches in out_off -> its first member and its rows; the rows of
//                       the call summed (64-bit).  Behind it an exclusive scan of the rows, and the call's one planning
//                       synchronisation: the total sizes the row tables
//   k_bgzf_range_rows   one lane per row: its range by a binary search in the scan, the member placed inside the bytes the
//                       range may read, gzip_head on the member's own bytes with the ISIZE the index implies, and the decoder's
//                       row exactly as k_bgzf_rows writes it (the stream is the FILE, implied entries and read limit absolute,
//                       kSegWrapped) beside its write window, its strip of one and its wrapper status; per range its span
//   k_bgzf_fold_spans   one wave per range: the first failing row in row order, a row's wrapper status before its body's
// No checksum is verified there (see sf_bgzf_range_plan.h).
#include "sf_bgzf_plan.h"
#include "sf_bgzf_range_plan.h"
#include "sf_device.h"

namespace sf {

namespace {

constexpr uint32_t KZ_THREADS = 256;
constexpr uint32_t KZ_LANE_BYTES = 32;
constexpr uint32_t KZ_BLOCK_BYTES = KZ_THREADS * KZ_LANE_BYTES;
constexpr uint32_t KZ_FIN = 1024;

inline uint32_t grid(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// WRITE = false: cnt[workgroup] = its nodes.  WRITE = true: the nodes, from node_off[workgroup] on.
template <bool WRITE>
__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_scan(const uint8_t* __restrict__ src, uint64_t n, uint32_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ node_off, uint64_t* __restrict__ pos,
                                                          uint32_t* __restrict__ size, uint32_t* __restrict__ isize) {
  __shared__ uint32_t s_wave[KZ_THREADS / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * KZ_BLOCK_BYTES + (uint64_t)t * KZ_LANE_BYTES;
  // the lane's 32 positions and the three bytes behind them: nine aligned dwords (src is 4-byte aligned; a dword that holds
  // a byte of the file is read whole, one that holds none is not read)
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
  uint32_t w[KZ_LANE_BYTES / 4 + 1];
#pragma unroll
  for (uint32_t k = 0; k <= KZ_LANE_BYTES / 4; ++k) w[k] = (p0 + 4 * k < n) ? s32[p0 / 4 + k] : 0u;
  uint32_t cand = 0, hits = 0;  // bit b: position p0 + b has the shape of a head / is a node
#pragma unroll
  for (uint32_t b = 0; b < KZ_LANE_BYTES; ++b)
    if (bgzf::head_shaped(__builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3))) cand |= 1u << b;
  while (cand) {  // (rare: three fixed bytes and a flag)
    const uint32_t b = (uint32_t)__ffs((int)cand) - 1;
    cand &= cand - 1;
    bgzf::Member M;
    if (p0 + b < n && bgzf::parse_member(src, n, p0 + b, M) == bgzf::kStOk) hits |= 1u << b;
  }
  const uint32_t mine = (uint32_t)__popc(hits);
  const uint32_t incl = wave_incl_add(mine);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t k = 0; k < KZ_THREADS / 64; ++k) {
    const uint32_t v = s_wave[k];
    before += k < wave ? v : 0u;
    all += v;
  }
  if constexpr (!WRITE) {
    if (t == 0) cnt[blockIdx.x] = all;
  } else {
    uint32_t at = node_off[blockIdx.x] + before + incl - mine;
    while (hits) {
      const uint32_t b = (uint32_t)__ffs((int)hits) - 1;
      hits &= hits - 1;
      bgzf::Member M;
      (void)bgzf::parse_member(src, n, p0 + b, M);
      pos[at] = p0 + b;
      size[at] = M.size;
      isize[at] = M.isize;
      ++at;
    }
  }
}

// nodes 0 .. nn - 1 and the sentinel nn
__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_succ(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ size, uint32_t nn,
                                                          uint32_t* __restrict__ nxt, uint32_t* __restrict__ hops,
                                                          uint8_t* __restrict__ mark) {
  const uint32_t i = blockIdx.x * KZ_THREADS + threadIdx.x;
  if (i > nn) return;
  if (i == nn) {
    nxt[i] = nn;
    hops[i] = 0;
    mark[i] = 0;
    return;
  }
  const uint64_t target = pos[i] + size[i];
  uint32_t lo = i + 1, hi = nn;  // (a member is 26 bytes at least: its successor lies behind it)
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pos[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  nxt[i] = (lo < nn && pos[lo] == target) ? lo : nn;
  hops[i] = 1;
  mark[i] = (i == 0 && pos[0] == 0) ? 1 : 0;
}

// One round: jumps and hops double (a -> b); a marked node marks the node its jump reaches.  Marks are only ever set on
// nodes of the chain from position 0 -- every jump is a composition of true successors -- so a mark set by another lane of
// the same round and seen early does no harm; after round k every chain node within 2^(k+1) - 1 hops of node 0 is marked.
__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_jump(const uint32_t* __restrict__ nxt_a, const uint32_t* __restrict__ hops_a,
                                                          uint32_t* __restrict__ nxt_b, uint32_t* __restrict__ hops_b,
                                                          uint8_t* mark, uint32_t nn) {
  const uint32_t i = blockIdx.x * KZ_THREADS + threadIdx.x;
  if (i > nn) return;
  const uint32_t j = nxt_a[i];
  if (i < nn && j < nn && mark[i]) mark[j] = 1;
  nxt_b[i] = nxt_a[j];
  hops_b[i] = hops_a[i] + hops_a[j];
}

struct BgzfWalk {     // k_bgzf_end -> k_bgzf_scatter, k_bgzf_finish
  uint32_t status;    // of the walk
  uint32_t members;
  uint32_t last;      // the chain's last node
  uint32_t pad;
};

__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_end(const uint8_t* __restrict__ src, uint64_t n, const uint64_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ size, const uint32_t* __restrict__ hops,
                                                         const uint8_t* __restrict__ mark, uint32_t nn, BgzfWalk* __restrict__ walk) {
  const uint32_t i = blockIdx.x * KZ_THREADS + threadIdx.x;
  bgzf::Member M;
  if (i == 0 && (nn == 0 || pos[0] != 0)) {  // nothing parses at byte 0 (n != 0: the host answers an empty file itself)
    const uint32_t st = bgzf::parse_member(src, n, 0, M);
    *walk = BgzfWalk{st ? st : bgzf::kStError, 0u, 0u, 0u};
    return;
  }
  if (i >= nn || !mark[i] || hops[i] != 1) return;
  const uint64_t end = pos[i] + size[i];
  uint32_t st = bgzf::kStOk;
  if (end != n) {  // (no node there, or the chain would go on: the member at `end` does not parse)
    st = bgzf::parse_member(src, n, end, M);
    st = st ? st : bgzf::kStError;
  }
  *walk = BgzfWalk{st, st ? 0u : hops[0], i, 0u};
}

__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_scatter(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ isize,
                                                             const uint32_t* __restrict__ hops, const uint8_t* __restrict__ mark,
                                                             uint32_t nn, const BgzfWalk* __restrict__ walk, uint64_t cap,
                                                             uint64_t* __restrict__ member_off, uint32_t* __restrict__ ranked) {
  const uint32_t i = blockIdx.x * KZ_THREADS + threadIdx.x;
  if (i >= nn || !mark[i]) return;
  const BgzfWalk W = *walk;
  if (W.status != bgzf::kStOk) return;
  const uint32_t r = hops[0] - hops[i];
  ranked[r] = isize[i];
  if ((uint64_t)W.members + 1 <= cap) member_off[r] = pos[i];
}

// One workgroup; every lane a run of consecutive members.
__global__ __launch_bounds__(KZ_FIN) void k_bgzf_finish(const uint8_t* __restrict__ src, uint64_t n, const uint64_t* __restrict__ pos,
                                                        const uint32_t* __restrict__ size, const uint32_t* __restrict__ ranked,
                                                        const BgzfWalk* __restrict__ walk, uint64_t cap,
                                                        uint64_t* __restrict__ member_off, uint64_t* __restrict__ out_off,
                                                        BgzfInfo* __restrict__ out) {
  __shared__ uint64_t s_sum[KZ_FIN];
  __shared__ uint32_t s_max[KZ_FIN];
  __shared__ uint32_t s_odd;
  const uint32_t t = threadIdx.x;
  const BgzfWalk W = *walk;
  if (W.status != bgzf::kStOk) {  // (uniform)
    if (t == 0) *out = BgzfInfo{0, 0, 0, 0, W.status, 0, 0, 0};
    return;
  }
  const uint32_t m = W.members, per = (m + KZ_FIN - 1) / KZ_FIN;
  const uint32_t i0 = min(t * per, m), i1 = min(i0 + per, m);
  uint64_t mine = 0;
  uint32_t widest = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint32_t v = ranked[i];
    mine += v;
    widest = max(widest, v);
  }
  s_sum[t] = mine;
  s_max[t] = widest;
  if (t == 0) s_odd = 0;
  __syncthreads();
  if (t == 0) {  // 1024 additions: the runs' sums into the bytes before each run
    uint64_t acc = 0;
    uint32_t mx = 0;
    for (uint32_t k = 0; k < KZ_FIN; ++k) {
      const uint64_t v = s_sum[k];
      s_sum[k] = acc;
      acc += v;
      mx = max(mx, s_max[k]);
    }
    s_max[0] = mx;
    const bool fits = (uint64_t)m + 1 <= cap;
    if (fits) {
      out_off[m] = acc;
      member_off[m] = n;
    }
    const uint32_t eof = bgzf::is_eof_member(src + pos[W.last], size[W.last]) ? 1u : 0u;
    *out = BgzfInfo{acc, m, mx, eof, bgzf::kStOk, fits ? 0 : bgzf::kDstTooSmall, 0, 0};
  }
  __syncthreads();
  if ((uint64_t)m + 1 > cap) return;  // (uniform)
  uint64_t o = s_sum[t];
  bool odd = false;
  for (uint32_t i = i0; i < i1; ++i) {
    out_off[i] = o;
    const uint32_t v = ranked[i];
    odd = odd || (v != 0 && (o & 15) != 0);
    o += v;
  }
  if (odd) atomicOr(&s_odd, 1u);
  __syncthreads();
  if (t == 0) out->unaligned = s_odd;
}

// sfh_decompress_bgzf_device: the first failing member in file order behind k_inflate_fold's statuses
__global__ __launch_bounds__(KZ_FIN) void k_bgzf_first(const uint32_t* __restrict__ status, uint32_t m, uint32_t* __restrict__ res) {
  __shared__ uint32_t s_first;
  const uint32_t t = threadIdx.x;
  if (t == 0) s_first = 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t i = t; i < m; i += KZ_FIN)
    if (status[i] != 0) {
      atomicMin(&s_first, i);
      break;
    }
  __syncthreads();
  if (t == 0) {
    res[0] = s_first == 0xFFFFFFFFu ? 0u : status[s_first];
    res[1] = s_first;
  }
}


constexpr uint32_t kNoMember = 0xFFFFFFFFu;  // plan[r] of a range the index does not hold

__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_range_spans(const BgzfRange* __restrict__ ranges, uint32_t n,
                                                                 const uint64_t* __restrict__ out_off, uint32_t members,
                                                                 uint32_t* __restrict__ plan, unsigned long long* __restrict__ total) {
  const uint32_t r = blockIdx.x * KZ_THREADS + threadIdx.x;
  uint32_t rows = 0;
  if (r < n) {
    const uint64_t off = ranges[r].offset, len = ranges[r].length;
    const bgzf::Span S = bgzf::span_of(out_off, members, off, len);
    // no rows: a range of no bytes inside the output, or one the index does not hold
    const bool held = len ? S.rows != 0 : bgzf::range_inside(out_off, members, off, len);
    plan[r] = held ? S.first : kNoMember;
    plan[n + r] = rows = held ? S.rows : 0u;
  }
  const uint32_t sum = wave_sum(rows);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, (unsigned long long)sum);
}

__global__ __launch_bounds__(KZ_THREADS) void k_bgzf_range_rows(const BgzfRange* __restrict__ ranges, uint32_t n,
                                                                const uint64_t* __restrict__ member_off,
                                                                const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ plan,
                                                                const uint32_t* __restrict__ row0, uint32_t nrows, uint32_t per_batch,
                                                                uint32_t row_bytes, InflateSeg* __restrict__ segs,
                                                                InflateClip* __restrict__ clips, InflateStrip* __restrict__ strips,
                                                                uint64_t* __restrict__ implied, uint32_t* __restrict__ wst,
                                                                InflateSpan* __restrict__ spans) {
  const uint32_t g = blockIdx.x * KZ_THREADS + threadIdx.x;
  if (g < n) spans[g] = InflateSpan{row0[g], plan[n + g]};  // (a range without rows has no row's lane: the first n lanes write the spans)
  if (g >= nrows) return;
  uint32_t lo = 0, hi = n - 1;  // the last range whose rows start at or before g: ranges without rows in front of it share its row0
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (row0[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  const BgzfRange R = ranges[lo];
  const bgzf::RangeRow W = bgzf::row_of(out_off, plan[lo], g - row0[lo], R.offset, R.length);
  const uint64_t a = member_off[W.member], e = member_off[W.member + 1];
  // the member inside the bytes this range may read, and no more output than a row holds -- else nothing of it is read
  uint32_t st = gz::kStOk, want = 0, isize = 0;
  uint64_t n_m = 0, hdr = 0, end = 0;
  if (a < R.src_lo || e < a || e > R.src_n || W.out_n > row_bytes) {
    st = gz::kStError;
  } else {
    n_m = end = e - a;
    gzip_head(R.src + a, n_m, W.out_n, st, hdr, end, want, isize);
    if (st == gz::kStOk && isize != W.out_n) st = gz::kStError;  // (above it: gzip_head's DstTooSmall)
  }
  const bool ok = st == gz::kStOk;
  uint64_t* ix = implied + 2 * (uint64_t)g;
  ix[0] = ok ? a + hdr : 0;
  ix[1] = ok ? a + end : 0;
  segs[g] = InflateSeg{R.src, ix, nullptr, nullptr, ok ? a + n_m - 8 : 0, ok ? W.out_n : 0u, kSegWrapped};
  clips[g] = InflateClip{R.dst + W.dst_off, ok ? W.lo : 0u, ok ? W.hi : 0u};
  strips[g] = InflateStrip{g % per_batch, 1u};
  wst[g] = st;
}

__global__ __launch_bounds__(64) void k_bgzf_fold_spans(const InflateSpan* __restrict__ spans, uint32_t n, const uint32_t* __restrict__ plan,
                                                        const SegInfo* __restrict__ info, const uint32_t* __restrict__ wst,
                                                        uint32_t* __restrict__ status) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  if (r >= n) return;
  const InflateSpan S = spans[r];
  uint32_t first = 0xFFFFFFFFu;
  for (uint32_t k = lane; k < S.nrows && first == 0xFFFFFFFFu; k += 64)
    if (wst[S.row0 + k] != gz::kStOk || info[S.row0 + k].status != 0) first = k;
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) first = min(first, (uint32_t)__shfl_xor((int)first, (int)d));
  if (lane != 0) return;
  uint32_t st = plan[r] == kNoMember ? gz::kStError : gz::kStOk;
  if (first != 0xFFFFFFFFu) st = wst[S.row0 + first] != gz::kStOk ? wst[S.row0 + first] : info[S.row0 + first].status;
  status[r] = st;
}

}  // namespace

uint32_t bgzf_scan_blocks(uint64_t src_n) { return grid(src_n, KZ_BLOCK_BYTES); }

hipError_t launch_bgzf_count(const uint8_t* src, uint64_t src_n, uint32_t* cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_scan<false>, dim3(bgzf_scan_blocks(src_n)), dim3(KZ_THREADS), 0, s, src, src_n, cnt, (const uint32_t*)nullptr,
                     (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  return hipGetLastError();
}

size_t bgzf_walk_bytes(uint32_t nn) {
  const size_t n1 = (size_t)nn + 1;
  // pos | size, isize, ranked | nxt a, b | hops a, b | the walk's result | marks
  return n1 * 8 + 3 * n1 * 4 + 4 * n1 * 4 + 16 + (n1 + 15) / 16 * 16;
}

hipError_t launch_bgzf_walk(const uint8_t* src, uint64_t src_n, const uint32_t* node_off, uint32_t nn, uint8_t* scratch,
                            uint64_t* member_off, uint64_t* out_off, uint64_t cap, BgzfInfo* out, hipStream_t s) {
  const size_t n1 = (size_t)nn + 1;
  uint64_t* pos = (uint64_t*)scratch;
  uint32_t* size = (uint32_t*)(pos + n1);
  uint32_t* isize = size + n1;
  uint32_t* ranked = isize + n1;
  uint32_t* nxt[2] = {ranked + n1, ranked + 2 * n1};
  uint32_t* hops[2] = {ranked + 3 * n1, ranked + 4 * n1};
  BgzfWalk* walk = (BgzfWalk*)(ranked + 5 * n1);
  uint8_t* mark = (uint8_t*)(walk + 1);
  int cur = 0;
  if (nn) {
    hipLaunchKernelGGL(k_bgzf_scan<true>, dim3(bgzf_scan_blocks(src_n)), dim3(KZ_THREADS), 0, s, src, src_n, (uint32_t*)nullptr, node_off,
                       pos, size, isize);
    hipLaunchKernelGGL(k_bgzf_succ, dim3(grid(n1, KZ_THREADS)), dim3(KZ_THREADS), 0, s, pos, size, nn, nxt[0], hops[0], mark);
    for (uint64_t reach = 1; reach <= nn; reach <<= 1, cur ^= 1)  // after the round: every node within 2 * reach - 1 hops
      hipLaunchKernelGGL(k_bgzf_jump, dim3(grid(n1, KZ_THREADS)), dim3(KZ_THREADS), 0, s, nxt[cur], hops[cur], nxt[cur ^ 1], hops[cur ^ 1],
                         mark, nn);
  }
  hipLaunchKernelGGL(k_bgzf_end, dim3(grid(n1, KZ_THREADS)), dim3(KZ_THREADS), 0, s, src, src_n, pos, size, hops[cur], mark, nn, walk);
  if (nn)
    hipLaunchKernelGGL(k_bgzf_scatter, dim3(grid(nn, KZ_THREADS)), dim3(KZ_THREADS), 0, s, pos, isize, hops[cur], mark, nn, walk, cap,
                       member_off, ranked);
  hipLaunchKernelGGL(k_bgzf_finish, dim3(1), dim3(KZ_FIN), 0, s, src, src_n, pos, size, ranked, walk, cap, member_off, out_off, out);
  return hipGetLastError();
}

hipError_t launch_bgzf_first(const uint32_t* status, uint32_t m, uint32_t* res, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_first, dim3(1), dim3(KZ_FIN), 0, s, status, m, res);
  return hipGetLastError();
}

hipError_t launch_bgzf_range_spans(const BgzfRange* ranges, uint32_t n, const uint64_t* out_off, uint32_t members, uint32_t* plan,
                                   unsigned long long* total, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(total, 0, sizeof *total, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bgzf_range_spans, dim3(grid(n, KZ_THREADS)), dim3(KZ_THREADS), 0, s, ranges, n, out_off, members, plan, total);
  return hipGetLastError();
}

hipError_t launch_bgzf_range_rows(const BgzfRange* ranges, uint32_t n, const uint64_t* member_off, const uint64_t* out_off,
                                  const uint32_t* plan, const uint32_t* row0, uint32_t nrows, uint32_t per_batch, uint32_t row_bytes,
                                  InflateSeg* segs, InflateClip* clips, InflateStrip* strips, uint64_t* implied, uint32_t* wst,
                                  InflateSpan* spans, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_range_rows, dim3(grid(nrows > n ? nrows : n, KZ_THREADS)), dim3(KZ_THREADS), 0, s, ranges, n, member_off,
                     out_off, plan, row0, nrows, per_batch, row_bytes, segs, clips, strips, implied, wst, spans);
  return hipGetLastError();
}

hipError_t launch_bgzf_fold_spans(const InflateSpan* spans, uint32_t n, const uint32_t* plan, const SegInfo* info, const uint32_t* wst,
                                  uint32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_fold_spans, dim3(n), dim3(64), 0, s, spans, n, plan, info, wst, status);
  return hipGetLastError();
}

}  // namespace sf
