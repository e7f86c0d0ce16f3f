// sf_checksum.hip -- CRC-32 (RFC 1952) and Adler-32 (RFC 1950) of the input on the GPU, and the
// zlib / gzip wrapper bytes around the raw DEFLATE stream (the reference's fixture
// tool deliberately strips the wrapper, /root/reference/tools/deflate_compress.py:8-13).
//
//   k_checksum<KIND>  one 256-thread workgroup per 32 KiB chunk, chunk staged through LDS
//                     (33-dword stride: conflict-free 128-byte thread segments); one u32 per chunk:
//                     CRC : remainder of chunk(x) * x^32 mod P with a zero register, the chunk
//                           zero-padded on the right to 32 KiB (so every chunk has the same length);
//                     Adler: (sum of weighted bytes mod 65521) << 16 | (sum of bytes mod 65521), weights
//                           counted from the padded chunk end.
//                     (CRC: table-driven per 128-byte thread segment, each remainder then multiplied by
//                     x^(8 * bytes behind it) mod P and all of them xor-ed)
//   k_wrap            one workgroup (k_wrap_batch: one per item of a batch): folds the per-chunk values in order (CRC: a tree of multiplications
//                     by x^(8*length) mod P, then the right padding is divided out with x^-1 and the
//                     0xFFFFFFFF preset / final inversion are applied; Adler: plain modular sums),
//                     writes the wrapper header and trailer, bumps the stream size.  With the call's index (SFH_DICTZIP) the
//                     gzip header carries the dictzip 'RA' table: the chunks' sizes, stored by all lanes.
//   k_dz_index        one workgroup: reads such a table back into a segment index (sf_dz_plan.h): one lane parses the
//                     header, all lanes load the sizes, a workgroup prefix sum, the index stored by all lanes.
//
//   k_bgzf_wrap       sfh_compress_bgzf*: one LANE per member (a chunk each): the chunk's CRC-32 finished from its partial,
//                     the 18-byte header with BSIZE from the offsets' difference, the trailer; the EOF member behind the last.
//   k_bgzf_rows       sfh_decompress_bgzf_device: one lane per member: k_inflate_head's gzip checks on the member's own bytes,
//                     and the decoder's rows -- the stream is the FILE (its base is aligned, a member's is not), the implied
//                     entries absolute.
//
// All arithmetic is integer; results are bit-exact with zlib's crc32()/adler32().
#include "sf_bgzf_plan.h"
#include "sf_device.h"
#include "sf_dz_plan.h"

namespace sf {

namespace {

constexpr uint32_t KC_THREADS = 256;
constexpr uint32_t KC_SEG = kChunk / KC_THREADS;      // 128 bytes per thread
constexpr uint32_t KC_SEGW = KC_SEG / 4;              // 32 dwords
constexpr uint32_t KC_STAGE = KC_THREADS * (KC_SEGW + 1);
constexpr uint32_t KW_THREADS = 1024;
constexpr uint32_t kAdlerMod = 65521u;

// GF(2)[x] mod P, reflected representation: bit 31 is x^0 (as in the CRC register)
__host__ __device__ constexpr uint32_t gf2_mulx(uint32_t b) { return (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1; }
__host__ __device__ constexpr uint32_t gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 31; k >= 0; --k) {
    p ^= ((a >> k) & 1u) ? b : 0u;
    b = gf2_mulx(b);
  }
  return p;
}
__host__ __device__ constexpr uint32_t gf2_pow(uint32_t base, uint64_t e) {
  uint32_t r = 0x80000000u;
  for (; e; e >>= 1) {
    if (e & 1) r = gf2_mul(r, base);
    base = gf2_mul(base, base);
  }
  return r;
}
constexpr uint32_t kX8 = 0x00800000u;     // x^8
constexpr uint32_t kXinv = 0xDB710641u;   // x^-1: gf2_mulx(kXinv) == x^0
static_assert(gf2_mulx(kXinv) == 0x80000000u, "x^-1");

// shift[t] = x^(8 * 128 * (255 - t)): carries thread t's segment remainder to the end of the chunk
struct SegShift {
  uint32_t shift[KC_THREADS];
};
constexpr SegShift make_seg_shift() {
  SegShift s{};
  const uint32_t seg = gf2_pow(kX8, KC_SEG);
  uint32_t v = 0x80000000u;
  for (int t = KC_THREADS - 1; t >= 0; --t) {
    s.shift[t] = v;
    v = gf2_mul(v, seg);
  }
  return s;
}
__constant__ SegShift c_seg = make_seg_shift();
constexpr uint32_t kChunkOp = gf2_pow(kX8, kChunk);  // x^(8*32768): appends one chunk

// the partial of one chunk: `valid` bytes at cp (16-byte aligned; ANY: of any alignment, read bytewise), zero-padded to kChunk,
// into *out
template <uint32_t KIND, bool ANY = false>
__device__ __forceinline__ void checksum_chunk(const uint8_t* __restrict__ cp, uint32_t valid, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_data[KC_STAGE];
  __shared__ uint32_t s_tab[KIND == kChecksumCrc32 ? 1024 : 1];
  __shared__ uint32_t s_part[KC_THREADS / 64][2];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // stage: dword d of the chunk -> s_data[d + d/32]; bytes past the end of the input are zero
  const uint4* s16 = reinterpret_cast<const uint4*>(cp);
#pragma unroll
  for (uint32_t i = 0; i < kChunk / 16 / KC_THREADS; ++i) {
    const uint32_t k = t + KC_THREADS * i, byte0 = 16 * k;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (!ANY && byte0 + 16 <= valid) {
      q = s16[k];
    } else if (byte0 < valid) {
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t b = 0; b < 16 && byte0 + b < valid; ++b) w[b >> 2] |= (uint32_t)cp[byte0 + b] << (8 * (b & 3));
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const uint32_t d = 4 * k, p = d + (d >> 5);
    s_data[p] = q.x;
    s_data[p + 1] = q.y;
    s_data[p + 2] = q.z;
    s_data[p + 3] = q.w;
  }

  if constexpr (KIND == kChecksumCrc32) {
    // slicing-by-4 tables: s_tab[256*j + b] = b(x) * x^(8*(j+1)) (register contents after j more zero bytes)
    uint32_t c = t;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = gf2_mulx(c);
    s_tab[t] = c;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 1; j < 4; ++j) {
      c = s_tab[c & 0xFF] ^ (c >> 8);
      s_tab[256 * j + t] = c;
    }
    __syncthreads();
    uint32_t r = 0;
    const uint32_t* seg = s_data + t * (KC_SEGW + 1);
#pragma unroll 8
    for (uint32_t j = 0; j < KC_SEGW; ++j) {
      r ^= seg[j];
      r = s_tab[768 + (r & 0xFF)] ^ s_tab[512 + ((r >> 8) & 0xFF)] ^ s_tab[256 + ((r >> 16) & 0xFF)] ^ s_tab[r >> 24];
    }
    // r(A||B) = r(A) * x^(8|B|) ^ r(B): every segment remainder is carried to the chunk end, then all are xor-ed
    r = gf2_mul(c_seg.shift[t], r);
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) r ^= __shfl_down(r, o);
    if (lane == 0) s_part[wave][0] = r;
    __syncthreads();
    if (t == 0) {
      uint32_t acc = 0;
      for (uint32_t w = 0; w < KC_THREADS / 64; ++w) acc ^= s_part[w][0];
      *out = acc;
    }
  } else {
    __syncthreads();
    uint32_t a = 0, b = 0;
    const uint32_t* seg = s_data + t * (KC_SEGW + 1);
#pragma unroll 8
    for (uint32_t j = 0; j < KC_SEGW; ++j) {
      const uint32_t w = seg[j], wt = KC_SEG - 4 * j;  // weights wt, wt-1, wt-2, wt-3 for bytes 0..3
      const uint32_t b0 = w & 0xFF, b1 = (w >> 8) & 0xFF, b2 = (w >> 16) & 0xFF, b3 = w >> 24;
      a += b0 + b1 + b2 + b3;
      b += wt * b0 + (wt - 1) * b1 + (wt - 2) * b2 + (wt - 3) * b3;
    }
    // weights counted from the padded chunk end: segment t is followed by (255 - t) * 128 bytes
    uint32_t bb = (b + (kChunk - KC_SEG * (t + 1)) * a) % kAdlerMod;  // < 2.2e6 + 32640 * 32640 < 2^32
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) {
      a += __shfl_down(a, o);
      bb += __shfl_down(bb, o);
    }
    if (lane == 0) {
      s_part[wave][0] = a;
      s_part[wave][1] = bb;
    }
    __syncthreads();
    if (t == 0) {
      uint32_t sa = 0, sb = 0;
      for (uint32_t w = 0; w < KC_THREADS / 64; ++w) {
        sa += s_part[w][0];
        sb += s_part[w][1];
      }
      *out = ((sb % kAdlerMod) << 16) | (sa % kAdlerMod);
    }
  }
}

template <uint32_t KIND>
__global__ __launch_bounds__(KC_THREADS) void k_checksum(const uint8_t* __restrict__ src, uint64_t n,
                                                         uint32_t* __restrict__ sums) {
  const uint64_t cbase = (uint64_t)blockIdx.x * kChunk;
  const uint32_t valid = (uint32_t)(n - cbase < kChunk ? n - cbase : kChunk);  // n == 0: one empty chunk
  checksum_chunk<KIND>(src + cbase, valid, sums + blockIdx.x);
}

// sfh_compress_batch*: chunk c of the call's chunk table (every item's chunks, in order)
template <uint32_t KIND>
__global__ __launch_bounds__(KC_THREADS) void k_checksum_batch(const BatchChunk* __restrict__ chunks, uint32_t* __restrict__ sums) {
  const BatchChunk B = chunks[blockIdx.x];
  checksum_chunk<KIND>(B.src, B.n_raw, sums + blockIdx.x);
}

// sfh_decompress_bgzf_device on a file whose ISIZEs leave a member's output off a 16-byte boundary
__global__ __launch_bounds__(KC_THREADS) void k_checksum_batch_any(const BatchChunk* __restrict__ chunks, uint32_t* __restrict__ sums) {
  const BatchChunk B = chunks[blockIdx.x];
  checksum_chunk<kChecksumCrc32, true>(B.src, B.n_raw, sums + blockIdx.x);
}

// sfh_compress_bgzf*: one lane per member of a launch batch, behind its k_emit and k_checksum.  Member c holds chunk c: its
// block lies at [offsets[c], offsets[c + 1] - 26) (k_scan with lead 18, extra 26), so the header goes 18 bytes in front of it
// and the trailer behind it.  The CRC-32 is wrap_stream's for a stream of one chunk: the zero padding divided out of the
// partial, the preset register carried over the chunk's bytes, the inversion -- only the batch's last member can be short,
// the others share kFullPreset.  n: the batch's input bytes.  eof: lane 0 stores the EOF member at *total and adds it
// (2: the file is that member alone, an empty input).  The members lie at any byte offset: single-byte stores.
constexpr uint32_t kFullPreset = gf2_mul(gf2_pow(kX8, kChunk), 0xFFFFFFFFu);
__global__ __launch_bounds__(256) void k_bgzf_wrap(const uint32_t* __restrict__ sums, const uint64_t* __restrict__ offsets,
                                                   uint32_t nmembers, uint64_t n, uint8_t* __restrict__ dst,
                                                   uint64_t* __restrict__ total, uint32_t eof) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c < nmembers) {
    const uint64_t cbase = (uint64_t)c * kChunk;
    const uint32_t m = (uint32_t)(n - cbase < kChunk ? n - cbase : kChunk);
    uint32_t raw = sums[c], preset = kFullPreset;
    if (m != kChunk) {
      raw = gf2_mul(raw, gf2_pow(kXinv, 8ull * (kChunk - m)));
      preset = gf2_mul(gf2_pow(kX8, m), 0xFFFFFFFFu);
    }
    const uint32_t crc = ~(raw ^ preset);
    const uint64_t b0 = offsets[c], b1 = offsets[c + 1];
    const uint32_t bsize = (uint32_t)(b1 - b0) - 1;  // (37504 + 26 at most: sfh_compress_bound's share of a chunk)
    uint8_t* h = dst + (b0 - bgzf::kHeader);
    for (uint32_t k = 0; k < 16; ++k) h[k] = bgzf::eof_byte(k);
    h[16] = (uint8_t)bsize;
    h[17] = (uint8_t)(bsize >> 8);
    uint8_t* tr = dst + (b1 - bgzf::kWrap);
    for (uint32_t k = 0; k < 4; ++k) {
      tr[k] = (uint8_t)(crc >> (8 * k));
      tr[4 + k] = (uint8_t)(m >> (8 * k));
    }
  }
  if (c == 0 && eof) {
    const uint64_t end = eof > 1 ? 0 : *total;
    for (uint32_t k = 0; k < bgzf::kEofBytes; ++k) dst[end + k] = bgzf::eof_byte(k);
    *total = end + bgzf::kEofBytes;
  }
}

// One workgroup.  total: in = header bytes + raw stream bytes (k_scan ran with that base), out += trailer.
// dst == nullptr: only *value is written (the checksum of the n input bytes).
// offsets (gzip only; null: the plain header): the call's index, nchunks + 1 entries -- the header is dictzip's, its table
// the differences of the entries (dst 4-byte aligned, so the table, at byte 22, takes 16-bit stores).
__device__ __forceinline__ void wrap_stream(const uint32_t* __restrict__ sums, uint32_t nchunks, uint64_t n, uint32_t kind,
                                            uint8_t* __restrict__ dst, uint64_t* __restrict__ total,
                                            uint32_t* __restrict__ value, uint32_t chunk_op,
                                            const uint64_t* __restrict__ offsets = nullptr) {
  __shared__ uint32_t s_v[KW_THREADS];
  __shared__ uint32_t s_w[KW_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nchunks + KW_THREADS - 1) / KW_THREADS;
  const uint64_t c0 = (uint64_t)t * per;
  uint32_t result = 0;
  if (kind == kChecksumCrc32) {
    uint32_t acc = 0;
    for (uint32_t k = 0; k < per; ++k) {
      const uint64_t c = c0 + k;
      const uint32_t v = c < nchunks ? sums[c] : 0u;  // chunks past the end: zero padding
      acc = (acc ? gf2_mul(chunk_op, acc) : 0u) ^ v;
    }
    s_v[t] = acc;
    uint32_t op = gf2_pow(kX8, (uint64_t)kChunk * per);  // appends one thread's range
    __syncthreads();
    for (uint32_t s = 1; s < KW_THREADS; s <<= 1) {
      if ((t & (2 * s - 1)) == 0) s_v[t] = gf2_mul(op, s_v[t]) ^ s_v[t + s];
      op = gf2_mul(op, op);
      __syncthreads();
    }
    if (t == 0) {
      const uint64_t pad = (uint64_t)KW_THREADS * per * kChunk - n;  // zero bytes appended above
      const uint32_t raw = gf2_mul(s_v[0], gf2_pow(kXinv, 8 * pad));
      result = ~(raw ^ gf2_mul(gf2_pow(kX8, n), 0xFFFFFFFFu));  // preset register, final inversion
    }
  } else {
    uint64_t sa = 0, sb = 0;
    for (uint32_t k = 0; k < per; ++k) {
      const uint64_t c = c0 + k;
      if (c >= nchunks) break;
      const uint32_t v = sums[c];
      const uint64_t a = v & 0xFFFF, b = v >> 16;
      const int64_t d = (int64_t)n - (int64_t)((c + 1) * kChunk);  // bytes after the padded chunk end (< 0: padding)
      const uint64_t dm = (uint64_t)((d % (int64_t)kAdlerMod + (int64_t)kAdlerMod) % (int64_t)kAdlerMod);
      sa += a;
      sb = (sb + b + dm * a) % kAdlerMod;
    }
    s_v[t] = (uint32_t)(sa % kAdlerMod);
    s_w[t] = (uint32_t)sb;
    __syncthreads();
    for (uint32_t s = KW_THREADS / 2; s; s >>= 1) {
      if (t < s) {
        s_v[t] += s_v[t + s];  // <= 1024 * 65520 < 2^32
        s_w[t] += s_w[t + s];
      }
      __syncthreads();
    }
    if (t == 0) {
      const uint32_t a = (1u + s_v[0]) % kAdlerMod;
      const uint32_t b = (uint32_t)((n % kAdlerMod + s_w[0]) % kAdlerMod);
      result = (b << 16) | a;
    }
  }
  if (dst && offsets) {
    // a chunk's size always fits 16 bits: sfh_compress_bound allows a 32 KiB block 32768 + 4096 + 640 = 37504 bytes
    uint16_t* tab = reinterpret_cast<uint16_t*>(dst + dz::kFixedHeader);
    for (uint32_t k = t; k < nchunks; k += KW_THREADS) tab[k] = (uint16_t)(offsets[k + 1] - offsets[k]);
  }
  if (t != 0) return;
  if (value) *value = result;
  if (!dst) return;
  const uint64_t end = *total;
  uint8_t* tr = dst + end;
  if (kind == kChecksumAdler32) {
    dst[0] = 0x78;  // CM 8, CINFO 7 (32 KiB window)
    dst[1] = 0x9C;  // FLEVEL 2, no FDICT, FCHECK
    tr[0] = (uint8_t)(result >> 24);
    tr[1] = (uint8_t)(result >> 16);
    tr[2] = (uint8_t)(result >> 8);
    tr[3] = (uint8_t)result;
    *total = end + 4;
  } else {
    const uint8_t h[10] = {0x1F, 0x8B, 8, (uint8_t)(offsets ? 4 : 0), 0, 0, 0, 0, 0, 0xFF};  // FEXTRA or no flags, MTIME 0, XFL 0, OS unknown
    for (int k = 0; k < 10; ++k) dst[k] = h[k];
    if (offsets) {  // XLEN | 'R' 'A' LEN | VER 1, CHLEN 32768, CHCNT (nchunks <= dz::kMaxChunks: the host checked)
      const uint32_t xlen = 10 + 2 * nchunks, len = 6 + 2 * nchunks;
      const uint8_t x[12] = {(uint8_t)xlen, (uint8_t)(xlen >> 8), 'R', 'A', (uint8_t)len, (uint8_t)(len >> 8), 1, 0,
                             (uint8_t)dz::kChunkLen, (uint8_t)(dz::kChunkLen >> 8), (uint8_t)nchunks, (uint8_t)(nchunks >> 8)};
      for (int k = 0; k < 12; ++k) dst[10 + k] = x[k];
    }
    const uint32_t isize = (uint32_t)n;
    for (int k = 0; k < 4; ++k) {
      tr[k] = (uint8_t)(result >> (8 * k));
      tr[4 + k] = (uint8_t)(isize >> (8 * k));
    }
    *total = end + 8;
  }
}

__global__ __launch_bounds__(KW_THREADS) void k_wrap(const uint32_t* __restrict__ sums, uint32_t nchunks, uint64_t n,
                                                     uint32_t kind, uint8_t* __restrict__ dst,
                                                     uint64_t* __restrict__ total, uint32_t* __restrict__ value,
                                                     uint32_t chunk_op, const uint64_t* __restrict__ offsets) {
  wrap_stream(sums, nchunks, n, kind, dst, total, value, chunk_op, offsets);
}

// sfh_dz_read_index_device: one workgroup.  Lane 0 parses the variable part of the header (sf_dz_plan.h); then every lane
// takes a run of consecutive sizes (at most 32: 32762 entries over 1024 lanes; byte loads, the table lies at any byte
// offset), the runs' sums are scanned over the wave (DPP) and the waves' totals through LDS, and every lane stores its run's
// index entries.  *out: the info, its last word the call's return code; the index is written only when both are 0.
__global__ __launch_bounds__(KW_THREADS) void k_dz_index(const uint8_t* __restrict__ src, uint64_t n, uint64_t* __restrict__ index,
                                                         uint64_t index_cap, DzInfo* __restrict__ out) {
  __shared__ dz::Head s_head;
  __shared__ int s_rc;
  __shared__ uint32_t s_wave[KW_THREADS / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) s_rc = dz::parse_head(src, n, s_head);
  __syncthreads();
  const dz::Head H = s_head;
  int rc = s_rc;
  uint32_t st = H.status;
  if (rc == dz::kOk && st == dz::kStOk) {  // (uniform)
    const uint32_t per = (H.chcnt + KW_THREADS - 1) / KW_THREADS;
    const uint32_t i0 = min(t * per, H.chcnt), i1 = min(i0 + per, H.chcnt);
    uint32_t mine = 0;  // (all sizes together stay below 2^32: 32762 * 65535)
    for (uint32_t i = i0; i < i1; ++i) mine += dz::size_at(src, H, i);
    const uint32_t incl = wave_incl_add(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < KW_THREADS / 64; ++w) {
      const uint32_t v = s_wave[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    if ((uint64_t)H.header_bytes + total > H.end) {
      st = dz::kStError;  // the sizes reach past the trailer
    } else if (index_cap < (uint64_t)H.nseg + 1) {
      rc = dz::kDstTooSmall;
    } else {
      uint64_t o = (uint64_t)H.header_bytes + before + (incl - mine);
      for (uint32_t i = i0; i < i1; ++i) {
        o += dz::size_at(src, H, i);
        if (i + 1 < H.nseg) index[i + 1] = o;  // (the last entry is the trailer's first byte, not the table's sum)
      }
      if (t == 0) {
        index[0] = H.header_bytes;
        index[H.nseg] = H.end;
      }
    }
  }
  if (t == 0) {
    const bool ok = rc == dz::kOk && st == dz::kStOk;
    *out = DzInfo{ok ? H.total_n : 0, ok ? H.nseg : 0u, ok ? H.header_bytes : 0u, st, rc};
  }
}

// sfh_compress_batch*: one workgroup per item, its own partials, header and trailer
__global__ __launch_bounds__(KW_THREADS) void k_wrap_batch(const uint32_t* __restrict__ sums, const WrapItem* __restrict__ items,
                                                           uint32_t kind, uint64_t* __restrict__ total, uint32_t chunk_op) {
  const WrapItem I = items[blockIdx.x];
  wrap_stream(sums + I.sum0, I.nchunks, I.n, kind, I.dst, total + I.out, nullptr, chunk_op);
}

// sfh_compress_zip*: the fold alone, one workgroup per item of a launch batch: the item's CRC-32 into crc[item.out]
__global__ __launch_bounds__(KW_THREADS) void k_crc_items(const uint32_t* __restrict__ sums, const WrapItem* __restrict__ items,
                                                          uint32_t* __restrict__ crc, uint32_t chunk_op) {
  const WrapItem I = items[blockIdx.x];
  wrap_stream(sums + I.sum0, I.nchunks, I.n, kChecksumCrc32, nullptr, nullptr, crc + I.out, chunk_op);
}

// ---- sfh_decompress_batch*: the wrappers of the items, and every item's status ----
// the reference's DecompressStatus values these kernels produce themselves (src/decompress.hpp:13-23)
constexpr uint32_t kStOk = 0, kStError = 1, kStSrcTooSmall = 5;

// (gzip_head, the gzip wrapper's checks: sf_device.h -- k_bgzf_range_rows of sf_bgzf.hip runs them as well)

// One lane per item, before the token kernels: the wrapper checks of include/starflate/container.hpp in its order (the
// header, the stream long enough for it, gzip's ISIZE against the output), the trailer's checksum, and with an index its
// first entry against the header's end.  An index-free call gets the item's one segment here: from the header's end to the
// trailer (nothing, for an item whose wrapper failed: its status is the wrapper's whatever the segment does).  A gzip item
// whose ISIZE is below its output size is decoded, as container.hpp decodes it, into the first ISIZE bytes only: its segment
// rows (segs) and checksum rows (sums) are cut down to them, and a body longer than that runs into DstTooSmall there.
__global__ __launch_bounds__(256) void k_inflate_head(InflateItem* __restrict__ items, uint32_t nitems, uint32_t kind,
                                                      InflateSeg* __restrict__ segs, BatchChunk* __restrict__ sums) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nitems) return;
  InflateItem& I = items[i];
  const uint8_t* p = I.src;
  const uint64_t n = I.src_n;
  uint32_t st = kStOk, want = 0, isize = 0;
  uint64_t hdr = 0, end = n;
  if (kind == kChecksumAdler32) {
    if (n < 6) {
      st = kStSrcTooSmall;
    } else {
      const uint32_t cmf = p[0], flg = p[1];
      if ((cmf & 0x0Fu) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20u) != 0) st = kStError;
      hdr = 2;
      end = n - 4;
      want = (uint32_t)p[n - 4] << 24 | (uint32_t)p[n - 3] << 16 | (uint32_t)p[n - 2] << 8 | p[n - 1];
    }
  } else if (kind == kChecksumCrc32) {
    gzip_head(p, n, I.dst_n, st, hdr, end, want, isize);
  }
  // (a raw item's index is the caller's business, as in sfh_decompress_device: its first entry need not be 0)
  if (kind != 0 && st == kStOk && I.ix0 && *I.ix0 != hdr) st = kStError;
  if (kind == kChecksumCrc32 && st == kStOk && isize < I.dst_n)
    for (uint32_t k = 0; k < I.nseg; ++k) {
      const uint64_t ob = (uint64_t)k * kChunk;
      const uint32_t on = isize > ob ? (isize - ob < kChunk ? (uint32_t)(isize - ob) : kChunk) : 0u;
      segs[I.seg0 + k].out_n = on;
      sums[I.seg0 + k].n_raw = on;
    }
  if (I.implied) {
    I.implied[0] = st == kStOk ? hdr : 0;
    I.implied[1] = st == kStOk ? end : 0;
  }
  I.wst = st;
  I.want = want;
  I.isize = isize;
}

// sfh_decompress_bgzf_device: one lane per member (its bytes [member_off[i], member_off[i + 1]) of the file, its output
// out_off[i] .. out_off[i + 1], at most 32768 bytes -- WIDE: 65536 --: one segment).  The member is an index-free gzip item of
// sfh_decompress_batch, checked by gzip_head on its own bytes -- but its segment row reads the FILE: the bit reader needs a
// 4-byte aligned base and takes any offset, so the implied entries (body start, trailer start) and the read limit are
// absolute.  Beside the segment row its write window (all of it: k_inflate_bytes_clip takes any destination alignment), its
// strip of one (numbered within its launch batch of `per_batch` rows) and its checksum row.
// WIDE (sfh_decompress_bgzf_wide_device): a member holds up to kWideRow bytes -- still one segment, in a wide row of the
// decoder, but TWO checksum rows, sums[2 i] its first kChunk bytes and sums[2 i + 1] the rest (empty for a member that has no
// more): the partials are per kChunk, and k_inflate_fold_wide folds the two.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_bgzf_rows(const uint8_t* __restrict__ src, const uint64_t* __restrict__ member_off,
                                                   const uint64_t* __restrict__ out_off, uint32_t nmembers, uint32_t per_batch,
                                                   uint8_t* __restrict__ dst, InflateSeg* __restrict__ segs,
                                                   InflateItem* __restrict__ items, InflateClip* __restrict__ clips,
                                                   InflateStrip* __restrict__ strips, BatchChunk* __restrict__ sums,
                                                   uint64_t* __restrict__ implied) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nmembers) return;
  const uint64_t a = member_off[i], n = member_off[i + 1] - a, o = out_off[i];
  const uint32_t on = (uint32_t)(out_off[i + 1] - o);
  uint32_t st = kStOk, want = 0, isize = 0;
  uint64_t hdr = 0, end = n;
  gzip_head(src + a, n, on, st, hdr, end, want, isize);
  uint64_t* ix = implied + 2 * (uint64_t)i;
  ix[0] = st == kStOk ? a + hdr : 0;
  ix[1] = st == kStOk ? a + end : 0;
  items[i] = InflateItem{src + a, n, on, ix, nullptr, i, 1u, st, want, isize, 0u};
  segs[i] = InflateSeg{src, ix, nullptr, dst + o, a + (n > 8 ? n - 8 : 0), on, kSegWrapped};
  clips[i] = InflateClip{dst + o, 0u, on};
  strips[i] = InflateStrip{i % per_batch, 1u};
  if constexpr (WIDE) {
    const uint32_t n0 = on < kChunk ? on : kChunk;
    sums[2 * (uint64_t)i] = BatchChunk{dst + o, n0, 0u};
    sums[2 * (uint64_t)i + 1] = BatchChunk{dst + o + n0, on - n0, 0u};
  } else {
    sums[i] = BatchChunk{dst + o, on, 0u};
  }
}

// One workgroup per item, behind every launch batch: the first failing segment in the item's stream order (what the serial
// decoder would report) after the wrapper's status; with a container and a clean body the checksum of the decoded bytes,
// folded from k_checksum_batch's partials by wrap_stream -- the compressor's fold -- against the trailer's.
// first (nullable): per item the number of that segment in the item, 0xFFFFFFFF when none failed (sfh_decompress_device's
// message names it).
// SUMS: checksum partials per segment record (2: wide rows of one segment per item, k_bgzf_rows<true>).
template <uint32_t SUMS>
__device__ __forceinline__ void inflate_fold(const InflateItem* __restrict__ items, const SegInfo* __restrict__ info,
                                             const uint32_t* __restrict__ sums, uint32_t kind,
                                             uint32_t* __restrict__ status, uint32_t* __restrict__ first,
                                             uint32_t chunk_op) {
  __shared__ uint32_t s_first, s_sum;
  const uint32_t t = threadIdx.x;
  const InflateItem I = items[blockIdx.x];
  if (t == 0) s_first = 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t k = t; k < I.nseg; k += KW_THREADS)
    if (info[I.seg0 + k].status != kStOk) {
      atomicMin(&s_first, k);
      break;
    }
  __syncthreads();
  const uint32_t f = s_first;
  uint32_t st = I.wst != kStOk ? I.wst : (f == 0xFFFFFFFFu ? kStOk : info[I.seg0 + f].status);
  if (kind != 0 && st == kStOk) {  // (uniform)
    // the checksum of what was decoded: gzip's first ISIZE bytes (k_inflate_head cut the rows down to them), else all
    const uint64_t n = (kind == kChecksumCrc32 && I.isize < I.dst_n) ? I.isize : I.dst_n;
    const uint32_t nch = n ? (uint32_t)((n + kChunk - 1) / kChunk) : 1u;
    wrap_stream(sums + (uint64_t)SUMS * I.seg0, nch, n, kind, nullptr, nullptr, &s_sum, chunk_op);
    __syncthreads();
    if (s_sum != I.want) st = kStError;
  }
  if (t == 0) {
    status[blockIdx.x] = st;
    if (first) first[blockIdx.x] = f;
  }
}

__global__ __launch_bounds__(KW_THREADS) void k_inflate_fold(const InflateItem* __restrict__ items, const SegInfo* __restrict__ info,
                                                             const uint32_t* __restrict__ sums, uint32_t kind,
                                                             uint32_t* __restrict__ status, uint32_t* __restrict__ first,
                                                             uint32_t chunk_op) {
  inflate_fold<1>(items, info, sums, kind, status, first, chunk_op);
}

__global__ __launch_bounds__(KW_THREADS) void k_inflate_fold_wide(const InflateItem* __restrict__ items, const SegInfo* __restrict__ info,
                                                                  const uint32_t* __restrict__ sums, uint32_t kind,
                                                                  uint32_t* __restrict__ status, uint32_t chunk_op) {
  inflate_fold<2>(items, info, sums, kind, status, nullptr, chunk_op);
}

}  // namespace

hipError_t launch_crc_items(const uint32_t* sums, const WrapItem* items, uint32_t nitems, uint32_t* crc, hipStream_t s) {
  hipLaunchKernelGGL(k_crc_items, dim3(nitems), dim3(KW_THREADS), 0, s, sums, items, crc, kChunkOp);
  return hipGetLastError();
}

hipError_t launch_inflate_head(InflateItem* items, uint32_t nitems, uint32_t container, InflateSeg* segs, BatchChunk* sums,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_inflate_head, dim3((nitems + 255) / 256), dim3(256), 0, s, items, nitems, container, segs, sums);
  return hipGetLastError();
}

hipError_t launch_inflate_fold(const InflateItem* items, uint32_t nitems, const SegInfo* info, const uint32_t* sums,
                               uint32_t container, uint32_t* status, uint32_t* first, hipStream_t s) {
  hipLaunchKernelGGL(k_inflate_fold, dim3(nitems), dim3(KW_THREADS), 0, s, items, info, sums, container, status, first, kChunkOp);
  return hipGetLastError();
}

hipError_t launch_inflate_fold_wide(const InflateItem* items, uint32_t nitems, const SegInfo* info, const uint32_t* sums,
                                    uint32_t container, uint32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_inflate_fold_wide, dim3(nitems), dim3(KW_THREADS), 0, s, items, info, sums, container, status, kChunkOp);
  return hipGetLastError();
}

// nseg: the call's segments, or 0 for the plain gzip header (the dictzip header carries a size per segment)
uint32_t wrapper_header_bytes(uint32_t kind, uint32_t nseg) {
  return kind == kChecksumAdler32 ? 2u : kind != kChecksumCrc32 ? 0u : nseg ? dz::kFixedHeader + 2 * nseg : 10u;
}

hipError_t launch_checksum(const uint8_t* src, uint64_t n, uint32_t nchunks, uint32_t kind, uint32_t* sums,
                           hipStream_t s) {
  if (kind == kChecksumCrc32)
    hipLaunchKernelGGL(k_checksum<kChecksumCrc32>, dim3(nchunks), dim3(KC_THREADS), 0, s, src, n, sums);
  else
    hipLaunchKernelGGL(k_checksum<kChecksumAdler32>, dim3(nchunks), dim3(KC_THREADS), 0, s, src, n, sums);
  return hipGetLastError();
}

hipError_t launch_wrap(const uint32_t* sums, uint32_t nchunks, uint64_t n, uint32_t kind, uint8_t* dst,
                       uint64_t* d_total, uint32_t* d_value, hipStream_t s, const uint64_t* dz_offsets) {
  hipLaunchKernelGGL(k_wrap, dim3(1), dim3(KW_THREADS), 0, s, sums, nchunks, n, kind, dst, d_total, d_value,
                     kChunkOp, dz_offsets);
  return hipGetLastError();
}

hipError_t launch_dz_index(const uint8_t* src, uint64_t src_n, uint64_t* index, uint64_t index_cap, DzInfo* out, hipStream_t s) {
  hipLaunchKernelGGL(k_dz_index, dim3(1), dim3(KW_THREADS), 0, s, src, src_n, index, index_cap, out);
  return hipGetLastError();
}

hipError_t launch_checksum_batch(const BatchChunk* chunks, uint32_t nchunks, uint32_t kind, uint32_t* sums, hipStream_t s) {
  if (kind == kChecksumCrc32)
    hipLaunchKernelGGL(k_checksum_batch<kChecksumCrc32>, dim3(nchunks), dim3(KC_THREADS), 0, s, chunks, sums);
  else
    hipLaunchKernelGGL(k_checksum_batch<kChecksumAdler32>, dim3(nchunks), dim3(KC_THREADS), 0, s, chunks, sums);
  return hipGetLastError();
}

hipError_t launch_checksum_batch_any(const BatchChunk* chunks, uint32_t nchunks, uint32_t* sums, hipStream_t s) {
  hipLaunchKernelGGL(k_checksum_batch_any, dim3(nchunks), dim3(KC_THREADS), 0, s, chunks, sums);
  return hipGetLastError();
}

hipError_t launch_bgzf_wrap(const uint32_t* sums, const uint64_t* offsets, uint32_t nmembers, uint64_t n, uint8_t* dst,
                            uint64_t* d_total, uint32_t eof, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_wrap, dim3(nmembers ? (nmembers + 255) / 256 : 1), dim3(256), 0, s, sums, offsets, nmembers, n, dst, d_total,
                     eof);
  return hipGetLastError();
}

hipError_t launch_bgzf_rows(const uint8_t* src, const uint64_t* member_off, const uint64_t* out_off, uint32_t nmembers,
                            uint32_t per_batch, uint8_t* dst, InflateSeg* segs, InflateItem* items, InflateClip* clips,
                            InflateStrip* strips, BatchChunk* sums, uint64_t* implied, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_rows<false>, dim3((nmembers + 255) / 256), dim3(256), 0, s, src, member_off, out_off, nmembers, per_batch, dst, segs,
                     items, clips, strips, sums, implied);
  return hipGetLastError();
}

hipError_t launch_bgzf_rows_wide(const uint8_t* src, const uint64_t* member_off, const uint64_t* out_off, uint32_t nmembers,
                                 uint32_t per_batch, uint8_t* dst, InflateSeg* segs, InflateItem* items, InflateClip* clips,
                                 InflateStrip* strips, BatchChunk* sums, uint64_t* implied, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_rows<true>, dim3((nmembers + 255) / 256), dim3(256), 0, s, src, member_off, out_off, nmembers, per_batch, dst,
                     segs, items, clips, strips, sums, implied);
  return hipGetLastError();
}

hipError_t launch_wrap_batch(const uint32_t* sums, const WrapItem* items, uint32_t nitems, uint32_t kind,
                             uint64_t* d_total, hipStream_t s) {
  hipLaunchKernelGGL(k_wrap_batch, dim3(nitems), dim3(KW_THREADS), 0, s, sums, items, kind, d_total, kChunkOp);
  return hipGetLastError();
}

uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return gf2_mul(gf2_pow(kX8, len_b), crc_a) ^ crc_b;
}

uint32_t adler32_combine(uint32_t adler_a, uint32_t adler_b, uint64_t len_b) {
  const uint64_t M = kAdlerMod;
  const uint64_t a1 = adler_a & 0xFFFF, b1 = adler_a >> 16, a2 = adler_b & 0xFFFF, b2 = adler_b >> 16;
  const uint64_t a = (a1 + a2 + M - 1) % M;
  const uint64_t b = (b1 + b2 + (len_b % M) * ((a1 + M - 1) % M)) % M;
  return (uint32_t)((b << 16) | a);
}

}  // namespace sf
