// sf_dz_plan.h -- the dictzip random-access table (dictzip(1): a gzip member whose FEXTRA field carries an 'RA' subfield
// with the compressed size of every independently coded chunk): the arithmetic of the header the compressor writes, and the
// parser that turns such a header into the decoder's segment index.  Plain C++, host and device: sf_checksum.hip runs the
// parser in k_dz_index, sf_capi.hip on host bytes, and the tests compile it for the host (tests/cpp/dz_index_host.cpp).
//
//   1F 8B 08 FLG MTIME(4) XFL OS | XLEN | subfields: SI1 SI2 LEN data | [FNAME] [FCOMMENT] [FHCRC] | body | CRC-32 ISIZE
//   'R' 'A' LEN = 6 + 2 * CHCNT | VER = 1 | CHLEN | CHCNT | CHCNT x u16 compressed bytes of chunk i        (all little-endian)
//
// The index (sfh_copy_index's convention): index[0] = the header's end, index[i + 1] = index[i] + size[i], and
// index[nseg] = src_n - 8, the trailer's first byte -- whatever lies between the table's end and the trailer (dictzip(1)
// leaves its empty final block there) belongs to the last segment.
// Every read is bounded by src_n: parse_head reads nothing it has not first placed inside [0, src_n - 8), the trailer is the
// last eight bytes, and size_at is only called for the entries parse_head found inside the extra field.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_DZ_HD __host__ __device__ inline
#else
#define SF_DZ_HD inline
#endif

namespace sf {
namespace dz {

constexpr uint32_t kChunkLen = 32768;    // CHLEN: the indexed decoder's segments (SFH_SEGMENT_BYTES)
constexpr uint32_t kMaxChunks = 32762;   // XLEN = 10 + 2 * CHCNT is 16 bits wide (SFH_DZ_MAX_CHUNKS)
constexpr uint64_t kMaxInput = (uint64_t)kMaxChunks * kChunkLen;
constexpr uint32_t kFixedHeader = 22;    // gzip header 10, XLEN 2, subfield header 4, VER CHLEN CHCNT 6

// the reference's DecompressStatus values the parser produces, and its two return codes (SFH_OK, SFH_E_NOT_INDEXABLE)
constexpr uint32_t kStOk = 0, kStError = 1, kStSrcTooSmall = 5;
constexpr int kOk = 0, kNotIndexable = -8;

SF_DZ_HD uint64_t chunks_of(uint64_t n) { return n ? (n + kChunkLen - 1) / kChunkLen : 1; }
// bytes of the header the compressor writes for n input bytes; 0 above the format's limit
SF_DZ_HD uint64_t header_bytes(uint64_t n) { return n > kMaxInput ? 0 : kFixedHeader + 2 * chunks_of(n); }

struct Head {
  uint64_t total_n;       // ISIZE
  uint64_t end;           // src_n - 8: the trailer's first byte
  uint64_t table;         // offset of the first chunk size
  uint32_t chcnt;         // sizes in the table (0: an empty input written without a chunk)
  uint32_t nseg;          // segments of the index: max(1, chcnt)
  uint32_t header_bytes;  // the header's end = index[0]
  uint32_t status;        // kStOk, kStError, kStSrcTooSmall
};

SF_DZ_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }  // (no alignment assumed)
SF_DZ_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
SF_DZ_HD uint32_t size_at(const uint8_t* src, const Head& H, uint32_t i) { return le16(src + H.table + 2 * (uint64_t)i); }

// Everything but the sizes' sum.  Returns kNotIndexable (H is then meaningless) or kOk with H.status: on kStOk the other
// fields are valid and the chcnt sizes lie inside the stream.
SF_DZ_HD int parse_head(const uint8_t* p, uint64_t n, Head& H) {
  H = Head{0, 0, 0, 0, 0, 0, kStOk};
  if (n < 18) {  // a gzip member is a header of 10 bytes and a trailer of 8 at least
    H.status = kStSrcTooSmall;
    return kOk;
  }
  if (p[0] != 0x1F || p[1] != 0x8B || p[2] != 8 || (p[3] & 0xE0u) != 0) {
    H.status = kStError;
    return kOk;
  }
  const uint32_t flg = p[3];
  if (!(flg & 0x04u)) return kNotIndexable;  // no FEXTRA
  const uint64_t end = n - 8;
  uint64_t at = 10;
  if (at + 2 > end || at + 2 + le16(p + at) > end) {  // XLEN overruns the stream
    H.status = kStError;
    return kOk;
  }
  const uint64_t xend = at + 2 + le16(p + at);
  at += 2;
  uint64_t ra = 0;
  uint32_t ra_len = 0;
  bool found = false;
  while (at < xend) {  // the subfields: others may stand before and behind 'RA' (the first 'RA' counts)
    if (at + 4 > xend || at + 4 + le16(p + at + 2) > xend) {  // a subfield overruns XLEN
      H.status = kStError;
      return kOk;
    }
    const uint32_t len = le16(p + at + 2);
    if (!found && p[at] == 'R' && p[at + 1] == 'A') {
      found = true;
      ra = at + 4;
      ra_len = len;
    }
    at += 4 + len;
  }
  if (!found) return kNotIndexable;
  for (uint32_t bit = 0x08u; bit <= 0x10u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (at < end && p[at] != 0) ++at;
    ++at;
  }
  if (flg & 0x02u) at += 2;  // FHCRC
  if (at > end) {            // the header does not fit in front of the trailer
    H.status = kStSrcTooSmall;
    return kOk;
  }
  if (ra_len < 6 || at > 0xFFFFFFFFull) {  // (header_bytes is 32 bits wide: no header with gigabytes of file name)
    H.status = kStError;
    return kOk;
  }
  if (le16(p + ra) != 1 || le16(p + ra + 2) != kChunkLen) return kNotIndexable;  // VER, CHLEN
  const uint32_t chcnt = le16(p + ra + 4);
  const uint32_t isize = le32(p + n - 4);
  if (ra_len != 6 + 2 * chcnt || (chcnt != chunks_of(isize) && !(chcnt == 0 && isize == 0))) {
    H.status = kStError;
    return kOk;
  }
  H.total_n = isize;
  H.end = end;
  H.table = ra + 6;
  H.chcnt = chcnt;
  H.nseg = chcnt ? chcnt : 1;
  H.header_bytes = (uint32_t)at;
  return kOk;
}

// The host's whole read: *status as Head::status (kStError as well when the sizes reach past the trailer).  Returns
// kNotIndexable, kOk, or kDstTooSmall when index_cap < nseg + 1; the index is written only on kOk with *status == kStOk.
constexpr int kDstTooSmall = -2;
inline int read_index(const uint8_t* p, uint64_t n, Head& H, uint64_t* index, uint64_t index_cap) {
  const int rc = parse_head(p, n, H);
  if (rc != kOk || H.status != kStOk) return rc;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < H.chcnt; ++i) sum += size_at(p, H, i);
  if (H.header_bytes + sum > H.end) {
    H.status = kStError;
    return kOk;
  }
  if (index_cap < (uint64_t)H.nseg + 1) return kDstTooSmall;
  uint64_t o = H.header_bytes;
  index[0] = o;
  for (uint32_t i = 0; i + 1 < H.nseg; ++i) index[i + 1] = o += size_at(p, H, i);
  index[H.nseg] = H.end;
  return kOk;
}

}  // namespace dz
}  // namespace sf
