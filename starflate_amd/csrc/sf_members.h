// sf_members.h -- multi-member gzip files (RFC 1952 2.2; SFH_GZIP_MEMBERS): the steps between one member's body and the next.
// Plain C++, host and device: the stream decoder's lanes run hop() where a body ends (sf_stream_core.h), k_stream_find runs
// head_candidate() on byte positions (sf_stream.hip), and the tests compile all three for the host against the specification,
// include/starflate/container.hpp's Container::GzipMembers case (tests/cpp/members_host.cpp).
//
//   member: 1F 8B 08 FLG MTIME(4) XFL OS | FEXTRA: XLEN(2) bytes | FNAME, FCOMMENT: zero-terminated | FHCRC(2) | body | CRC-32 ISIZE
//   file:   member { zero bytes } member ... { zero bytes }
//
// Every read is bounded by n, the file's bytes: a field is placed inside the file before anything in it is read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_MEMBERS_HD __host__ __device__ inline
#else
#define SF_MEMBERS_HD inline
#endif

namespace sf {
namespace members {

// the reference's DecompressStatus values these steps produce
constexpr uint32_t kStOk = 0, kStError = 1, kStSrcTooSmall = 5;

SF_MEMBERS_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }  // (no alignment assumed)
SF_MEMBERS_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

// The gzip header at byte `at` of the n bytes at p (at <= n): container.hpp's checks in its order, on the bytes [at, n).
// st == kStOk: returns the header's end, the body's first byte, at most n - 8.  Else st is the status and the value means nothing.
SF_MEMBERS_HD uint64_t header_end(const uint8_t* p, uint64_t at, uint64_t n, uint32_t& st) {
  st = kStOk;
  if (n - at < 18) {
    st = kStSrcTooSmall;
    return at;
  }
  const uint8_t* h = p + at;
  if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || (h[3] & 0xE0u) != 0) {
    st = kStError;
    return at;
  }
  const uint32_t flg = h[3];
  const uint64_t end = n - 8;
  uint64_t q = at + 10;
  if (flg & 0x04u) {  // FEXTRA
    if (q + 2 > end) {
      st = kStSrcTooSmall;
      return at;
    }
    q += 2 + le16(p + q);
  }
  for (uint32_t bit = 0x08u; bit <= 0x10u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (q < end && p[q] != 0) ++q;
    ++q;
  }
  if (flg & 0x02u) q += 2;  // FHCRC
  if (q > end) st = kStSrcTooSmall;
  return q;
}

struct Hop {
  uint64_t src_end;  // the byte just past the trailer
  uint64_t next;     // !end && st == kStOk: the next body's first byte
  uint32_t crc32, isize;
  uint32_t st;
  uint32_t end;      // 1: only zero bytes, or nothing, lie behind the trailer: the file's end
};

// From the bit just past a body's last (a bit offset into p, at most 8 n) to the next body: byte-align, the 8 trailer bytes,
// the zero bytes behind them, then the file's end or the next member's header.  The trailer's values are read, not checked.
SF_MEMBERS_HD Hop hop(const uint8_t* p, uint64_t n, uint64_t body_end_bit) {
  Hop h{0, 0, 0, 0, kStOk, 0};
  uint64_t at = (body_end_bit + 7) >> 3;
  if (n - at < 8) {
    h.st = kStSrcTooSmall;
    return h;
  }
  h.crc32 = le32(p + at);
  h.isize = le32(p + at + 4);
  at += 8;
  h.src_end = at;
  while (at < n && p[at] == 0) ++at;
  if (at == n) {
    h.end = 1;
    return h;
  }
  h.next = header_end(p, at, n, h.st);
  return h;
}

// does a member's head stand at byte `at` (at < n): the magic, CM 8, clear reserved FLG bits and a header that parses
SF_MEMBERS_HD bool head_candidate(const uint8_t* p, uint64_t at, uint64_t n) {
  if (n - at < 18 || p[at] != 0x1F || p[at + 1] != 0x8B || p[at + 2] != 8 || (p[at + 3] & 0xE0u) != 0) return false;
  uint32_t st;
  header_end(p, at, n, st);
  return st == kStOk;
}

}  // namespace members
}  // namespace sf
