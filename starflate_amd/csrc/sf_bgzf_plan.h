// sf_bgzf_plan.h -- BGZF, the blocked gzip of bgzip / htslib (BAM, BCF, tabix): a series of complete gzip members of at most
// 64 KiB, each stating its own compressed size in a 'BC' extra subfield, closed by a fixed empty member.  The arithmetic of
// what the compressor writes, and the parser that finds the members.  Plain C++, host and device: sf_bgzf.hip runs
// parse_member on every byte position that looks like a member's head, sf_capi.hip walks host bytes with read_index, and the
// tests compile it for the host (tests/cpp/bgzf_index_host.cpp).
//
//   member: 1F 8B 08 FLG(FEXTRA set) MTIME(4) XFL OS | XLEN | subfields: SI1 SI2 SLEN data | body | CRC-32 ISIZE
//           'B' 'C' SLEN = 2 | BSIZE = the member's bytes - 1                                              (all little-endian)
//   EOF:    the member of an empty input with a fixed-Huffman body (03 00), 28 bytes
//
// A member the compressor writes has XLEN = 6 (the 'BC' subfield alone), so its body starts at byte 18.  Others may carry
// further subfields before and behind 'BC'; FNAME, FCOMMENT and FHCRC are the gzip decoder's business (k_inflate_head skips
// them), the parser only needs the member's length and its ISIZE, the last four bytes.
// Every read is bounded by src_n: the fixed twelve bytes, then the extra field, then the member's end are each placed
// inside the file before anything in them is read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_BGZF_HD __host__ __device__ inline
#else
#define SF_BGZF_HD inline
#endif

namespace sf {
namespace bgzf {

constexpr uint32_t kMemberInput = 32768;  // input bytes per member the compressor writes: one chunk, one DEFLATE block
constexpr uint32_t kHeader = 18;          // gzip header 10, XLEN 2, 'B' 'C' SLEN 4, BSIZE 2
constexpr uint32_t kWrap = kHeader + 8;   // ... and the trailer: what a member adds to its body
constexpr uint32_t kEofBytes = 28;
constexpr uint32_t kMaxMember = 65536;    // BSIZE is 16 bits wide
// byte k of the EOF member; its first sixteen bytes are those of every member the compressor writes (BSIZE follows them)
SF_BGZF_HD uint8_t eof_byte(uint32_t k) {
  const uint8_t e[kEofBytes] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 'B', 'C', 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return e[k];
}

// the reference's DecompressStatus values the parser produces, and read_index's return codes (SFH_OK, SFH_E_DST_TOO_SMALL)
constexpr uint32_t kStOk = 0, kStError = 1, kStSrcTooSmall = 5;
constexpr int kOk = 0, kDstTooSmall = -2;

// members of the file the compressor writes for n input bytes (the EOF member not counted), and the largest such file:
// every member's body within sfh_compress_bound's share of one chunk
SF_BGZF_HD uint64_t members_of(uint64_t n) { return (n + kMemberInput - 1) / kMemberInput; }
SF_BGZF_HD uint64_t bound(uint64_t n) {
  const uint64_t m = members_of(n) ? members_of(n) : 1;
  return m * (uint64_t)(kMemberInput + kMemberInput / 8 + 640 + kWrap) + kEofBytes;
}

// The reader's wide rows (a file with a member above kMemberInput bytes of output; kMaxMember at most).  A wide member's tokens
// take twice a narrow one's scratch, so a launch batch of `batch_chunks` narrow members holds half as many wide ones (one at
// least); and the checksum partials stay per kMemberInput bytes: two rows per wide member, 2 i and 2 i + 1.
SF_BGZF_HD uint32_t wide_batch(uint32_t batch_chunks) { return batch_chunks / 2 ? batch_chunks / 2 : 1u; }
SF_BGZF_HD uint64_t checksum_rows(uint64_t members, bool wide) { return wide ? 2 * members : members; }

SF_BGZF_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }  // (no alignment assumed)
SF_BGZF_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

struct Member {
  uint32_t size;    // BSIZE + 1: the member's bytes
  uint32_t isize;   // its last four bytes
  uint32_t header;  // 12 + XLEN: the extra field's end
};

// bytes at[0..2] = 1F 8B 08 and FEXTRA set: what the device scan tests at every position before it parses
SF_BGZF_HD bool head_shaped(uint32_t first4) { return (first4 & 0x04FFFFFFu) == 0x04088B1Fu; }

// The member that starts at byte `at` of the n bytes at p (at <= n).  kStOk: M is valid and the member lies inside the file.
// kStSrcTooSmall: its header or its BSIZE + 1 bytes reach past n.  kStError: bad magic or CM, FEXTRA clear, a subfield that
// overruns XLEN, no 'BC' subfield of two bytes, or BSIZE + 1 below the header and the trailer.
SF_BGZF_HD uint32_t parse_member(const uint8_t* p, uint64_t n, uint64_t at, Member& M) {
  M = Member{0, 0, 0};
  if (n - at < 12) return kStSrcTooSmall;  // the fixed header and XLEN
  const uint8_t* h = p + at;
  if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || !(h[3] & 0x04u)) return kStError;
  const uint32_t xlen = le16(h + 10);
  if (n - at < 12ull + xlen) return kStSrcTooSmall;
  uint32_t x = 0, bsize = 0;
  bool found = false;
  while (x < xlen) {  // the subfields: others may stand before and behind 'BC' (the first 'BC' of two bytes counts)
    if (x + 4 > xlen || x + 4 + le16(h + 12 + x + 2) > xlen) return kStError;
    const uint32_t slen = le16(h + 12 + x + 2);
    if (!found && h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2) {
      found = true;
      bsize = le16(h + 12 + x + 4);
    }
    x += 4 + slen;
  }
  if (!found) return kStError;
  const uint32_t size = bsize + 1;
  if (size < 12 + xlen + 8) return kStError;
  if (n - at < size) return kStSrcTooSmall;
  M = Member{size, le32(h + size - 4), 12 + xlen};
  return kStOk;
}

SF_BGZF_HD bool is_eof_member(const uint8_t* p, uint32_t size) {
  if (size != kEofBytes) return false;
  for (uint32_t k = 0; k < kEofBytes; ++k)
    if (p[k] != eof_byte(k)) return false;
  return true;
}

struct Info {
  uint64_t total_n;    // the members' ISIZEs together
  uint32_t members;    // the EOF member and every other empty member count
  uint32_t max_isize;
  uint32_t has_eof;    // the last member is byte for byte the EOF member
  uint32_t status;     // kStOk, kStError, kStSrcTooSmall: of the first member that does not parse
};

// The host's walk, member after member.  member_off[0 .. members] = every member's first byte and n; out_off[0 .. members] =
// the prefix sums of ISIZE.  Returns kDstTooSmall when cap < members + 1 (I then holds the counts: what to allocate); the
// arrays are written only on kOk with status kStOk, and with another status the counts are 0.
inline int read_index(const uint8_t* p, uint64_t n, Info& I, uint64_t* member_off, uint64_t* out_off, uint64_t cap) {
  I = Info{0, 0, 0, 0, kStOk};
  for (int pass = 0; pass < 2; ++pass) {  // count and check, then write
    uint64_t at = 0, out = 0;
    uint32_t m = 0, widest = 0, last = 0;
    while (at < n) {
      Member M;
      const uint32_t st = parse_member(p, n, at, M);
      if (st != kStOk) {
        I.status = st;
        return kOk;
      }
      if (pass) {
        member_off[m] = at;
        out_off[m] = out;
      }
      last = M.size;
      widest = M.isize > widest ? M.isize : widest;
      at += M.size;
      out += M.isize;
      ++m;
    }
    if (pass) {
      member_off[m] = n;
      out_off[m] = out;
      return kOk;
    }
    I = Info{out, m, widest, (m && is_eof_member(p + n - last, last)) ? 1u : 0u, kStOk};
    if (cap < (uint64_t)m + 1) return kDstTooSmall;
  }
  return kOk;
}

}  // namespace bgzf
}  // namespace sf
