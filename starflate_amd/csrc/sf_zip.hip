// sf_zip.hip -- ZIP archives (sf_zip_plan.h): the kernels of the reader and the writer.
//   k_zip_locals   sfh_zip_read_index_device: one lane per entry of the table the host walked out of the central directory:
//                  parse_local on the device file -> data_off and the entry's status
//   k_zip_store    sfh_decompress_zip*: the gather copy of stored entries, one workgroup per 32 KiB piece of one entry
//   k_zip_place    sfh_compress_zip*: behind a launch batch's k_emit, the exclusive scan of 30 + name_len + out_n over its items,
//                  carried on from the batches before it: where every local header goes
//   k_zip_pack     ... one workgroup per 32 KiB piece of an item's raw stream: from its scratch slot to its place in the archive,
//                  the local header and the name in front of piece 0
//   k_zip_wrap     ... behind the last launch batch: one lane per entry writes its directory record, lane 0 the end record(s)
//                  and the archive's size
// The CRC-32 of the reader is k_checksum_batch's partials (one per 32 KiB piece of an entry's output) folded per entry by
// k_inflate_fold against the directory's value -- the gzip items' kernels and arithmetic (sf_checksum.hip); the writer's is
// k_checksum_batch over the items' chunks and k_crc_items' fold.
// A copy moves 16 bytes per lane and step: the destination side is 16-byte aligned (k_zip_store: by contract; k_zip_pack: after
// up to 15 head bytes), the source side is read as the two aligned 16-byte words around it and put together in registers
// (v_alignbyte_b32, the idiom of k_bgzf_scan).  No load touches a byte outside [lo, hi), the caller's statement of what is
// readable around the source (the file up to the dword that holds its last byte; an item's scratch slot), and no store a byte
// outside the n destination bytes.
#include "sf_device.h"
#include "sf_zip_plan.h"

namespace sf {
namespace {

constexpr uint32_t KZP_THREADS = 256;

// out = bytes [sh, sh + 16) of the 32 bytes a | b (sh = 4 d + r; uniform over a workgroup: one source, one destination)
__device__ __forceinline__ uint4 join16(uint4 a, uint4 b, uint32_t sh) {
  const uint32_t d = sh >> 2, r = sh & 3;
  uint32_t w0, w1, w2, w3, w4;
  switch (d) {
    case 0: w0 = a.x; w1 = a.y; w2 = a.z; w3 = a.w; w4 = b.x; break;
    case 1: w0 = a.y; w1 = a.z; w2 = a.w; w3 = b.x; w4 = b.y; break;
    case 2: w0 = a.z; w1 = a.w; w2 = b.x; w3 = b.y; w4 = b.z; break;
    default: w0 = a.w; w1 = b.x; w2 = b.y; w3 = b.z; w4 = b.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r),
                    __builtin_amdgcn_alignbyte(w3, w2, r), __builtin_amdgcn_alignbyte(w4, w3, r));
}

// n bytes from src to dst, both of any alignment, by the whole workgroup.  [lo, hi): the addresses around src that may be
// loaded (16-byte loads stay inside; what lies closer to an edge than that goes bytewise).
__device__ __forceinline__ void copy_piece(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uintptr_t lo,
                                           uintptr_t hi) {
  const uint32_t t = threadIdx.x;
  const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
  if (t < head) dst[t] = src[t];
  const uint32_t full = (n - head) / 16;
  const uint8_t* s0 = src + head;
  uint4* d16 = reinterpret_cast<uint4*>(dst + head);
  const uint32_t sh = (uint32_t)((uintptr_t)s0 & 15);
  for (uint32_t k = t; k < full; k += KZP_THREADS) {
    const uint8_t* s = s0 + 16 * (size_t)k;
    const uintptr_t a = (uintptr_t)s - sh;  // the aligned word that holds the chunk's first byte
    uint4 q;
    if (a >= lo && a + (sh ? 32 : 16) <= hi) {
      const uint4 x = *reinterpret_cast<const uint4*>(a);
      q = sh ? join16(x, *reinterpret_cast<const uint4*>(a + 16), sh) : x;
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t b = 0; b < 16; ++b) w[b >> 2] |= (uint32_t)s[b] << (8 * (b & 3));
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    d16[k] = q;
  }
  const uint32_t done = head + 16 * full;
  if (t < n - done) dst[done + t] = src[done + t];
}

__global__ __launch_bounds__(256) void k_zip_locals(const uint8_t* __restrict__ src, uint64_t limit, zip::Entry* __restrict__ entries,
                                                    uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  zip::Entry E = entries[i];
  zip::parse_local(src, limit, E);
  entries[i].data_off = E.data_off;
  entries[i].status = E.status;
}

__global__ __launch_bounds__(KZP_THREADS) void k_zip_store(const ZipCopy* __restrict__ rows, const ZipPiece* __restrict__ pieces,
                                                           uintptr_t lo, uintptr_t hi) {
  const ZipPiece P = pieces[blockIdx.x];
  const ZipCopy R = rows[P.row];
  const uint64_t at = (uint64_t)P.piece * zip::kPiece;
  const uint32_t n = (uint32_t)(R.n - at < zip::kPiece ? R.n - at : zip::kPiece);
  copy_piece(R.dst + at, row_ptr(R.src) + at, n, lo, hi);
}

// One workgroup: off[i] = *carry + the sum of 30 + name_len + out_n over the items before i; *carry += the sum over all.
__global__ __launch_bounds__(1024) void k_zip_place(const ZipItem* __restrict__ items, const uint64_t* __restrict__ out_n, uint32_t n,
                                                    uint64_t* __restrict__ off, uint64_t* __restrict__ carry) {
  __shared__ uint64_t s_sum[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
  const uint32_t i0 = min(n, t * per), i1 = min(n, i0 + per);
  uint64_t mine = 0;
  for (uint32_t i = i0; i < i1; ++i) mine += zip::kLocal + items[i].name_len + out_n[i];
  s_sum[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan of the lanes' sums
    const uint64_t v = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint64_t o = *carry + s_sum[t] - mine;
  for (uint32_t i = i0; i < i1; ++i) {
    off[i] = o;
    o += zip::kLocal + items[i].name_len + out_n[i];
  }
  __syncthreads();  // (every lane has read *carry)
  if (t == 1023) *carry = *carry + s_sum[1023];
}

// slots: the items' raw streams in the context's scratch, item i's at slots + slot_off[i] (16-byte aligned, slot_n[i] bytes)
__global__ __launch_bounds__(KZP_THREADS) void k_zip_pack(const ZipItem* __restrict__ items, const ZipPiece* __restrict__ pieces,
                                                          const uint8_t* __restrict__ names, const uint64_t* __restrict__ out_n,
                                                          const uint64_t* __restrict__ off, const uint32_t* __restrict__ crc,
                                                          const uint8_t* __restrict__ slots, uint8_t* __restrict__ dst) {
  const ZipPiece P = pieces[blockIdx.x];
  const ZipItem I = items[P.row];
  const uint64_t body = out_n[P.row], at = (uint64_t)P.piece * zip::kPiece;
  uint8_t* d = dst + off[P.row];
  if (P.piece == 0) {
    const uint8_t* nm = names + I.name_off;
    if (threadIdx.x == 0) {  // (the name itself: by all lanes)
      zip::write_local(d, nm, 0, crc[P.row], (uint32_t)body, I.usize);
      zip::st16(d + 26, I.name_len);
    }
    for (uint32_t k = threadIdx.x; k < I.name_len; k += KZP_THREADS) d[zip::kLocal + k] = nm[k];
  }
  if (at >= body) return;  // (the pieces cover the item's bound)
  const uint32_t n = (uint32_t)(body - at < zip::kPiece ? body - at : zip::kPiece);
  const uint8_t* slot = slots + I.slot_off;
  copy_piece(d + zip::kLocal + I.name_len + at, slot + at, n, (uintptr_t)slot, (uintptr_t)slot + I.slot_n);
}

// names_n: the names' bytes together; *carry: the directory's first byte (the end of the last local part)
__global__ __launch_bounds__(256) void k_zip_wrap(const ZipItem* __restrict__ items, const uint8_t* __restrict__ names,
                                                  const uint64_t* __restrict__ out_n, const uint64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ crc, uint64_t n, uint64_t names_n,
                                                  const uint64_t* __restrict__ carry, uint8_t* __restrict__ dst,
                                                  uint64_t* __restrict__ total) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t cd_off = *carry, cd_size = zip::kCentral * n + names_n;
  if (i < n) {
    const ZipItem I = items[i];
    zip::write_central(dst + cd_off + zip::kCentral * i + I.name_off, names + I.name_off, I.name_len, crc[i], (uint32_t)out_n[i],
                       I.usize, (uint32_t)off[i]);
  }
  if (i == 0) *total = cd_off + cd_size + zip::write_end(dst + cd_off + cd_size, n, cd_off, cd_size);
}

inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

hipError_t launch_zip_locals(const uint8_t* src, uint64_t limit, zip::Entry* entries, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_zip_locals, dim3(blocks_of(n, 256)), dim3(256), 0, s, src, limit, entries, n);
  return hipGetLastError();
}

hipError_t launch_zip_store(const ZipCopy* rows, const ZipPiece* pieces, uint32_t npieces, const uint8_t* file, uint64_t file_n,
                            hipStream_t s) {
  if (npieces == 0) return hipSuccess;
  const uintptr_t lo = (uintptr_t)file, hi = lo + ((file_n + 3) & ~(uint64_t)3);
  hipLaunchKernelGGL(k_zip_store, dim3(npieces), dim3(KZP_THREADS), 0, s, rows, pieces, lo, hi);
  return hipGetLastError();
}

hipError_t launch_zip_place(const ZipItem* items, const uint64_t* out_n, uint32_t n, uint64_t* off, uint64_t* carry, hipStream_t s) {
  hipLaunchKernelGGL(k_zip_place, dim3(1), dim3(1024), 0, s, items, out_n, n, off, carry);
  return hipGetLastError();
}

hipError_t launch_zip_pack(const ZipItem* items, const ZipPiece* pieces, uint32_t npieces, const uint8_t* names, const uint64_t* out_n,
                           const uint64_t* off, const uint32_t* crc, const uint8_t* slots, uint8_t* dst, hipStream_t s) {
  if (npieces == 0) return hipSuccess;
  hipLaunchKernelGGL(k_zip_pack, dim3(npieces), dim3(KZP_THREADS), 0, s, items, pieces, names, out_n, off, crc, slots, dst);
  return hipGetLastError();
}

hipError_t launch_zip_wrap(const ZipItem* items, const uint8_t* names, const uint64_t* out_n, const uint64_t* off, const uint32_t* crc,
                           uint64_t n, uint64_t names_n, const uint64_t* carry, uint8_t* dst, uint64_t* total, hipStream_t s) {
  hipLaunchKernelGGL(k_zip_wrap, dim3(n ? blocks_of(n, 256) : 1u), dim3(256), 0, s, items, names, out_n, off, crc, n, names_n, carry,
                     dst, total);
  return hipGetLastError();
}

}  // namespace sf
