// sf_zip_plan.h -- ZIP (APPNOTE 6.3; .zip, .npz, .jar, .whl, .docx, torch.save): the archive layer around stored (method 0)
// and deflated (method 8) entries.  The parser that finds the end record, walks the central directory and places every
// entry's data, and the arithmetic of what the writer stores.  Plain C++, host and device: sf_zip.hip runs parse_local on the
// device file and the writers behind every launch batch, sf_capi.hip walks host bytes with read_index, and the tests compile
// it for the host (tests/cpp/zip_index_host.cpp).
//
//   local header  50 4B 03 04 | need(2) flags(2) method(2) time(2) date(2) | crc(4) csize(4) usize(4) | nlen(2) xlen(2) | name extra
//   directory     50 4B 01 02 | made(2) need(2) flags(2) method(2) time(2) date(2) | crc(4) csize(4) usize(4) |
//                 nlen(2) xlen(2) clen(2) disk(2) iattr(2) xattr(4) local_off(4) | name extra comment
//   end record    50 4B 05 06 | disk(2) cd_disk(2) here(2) entries(2) | cd_size(4) cd_off(4) | clen(2) comment
//   ZIP64 end     50 4B 06 06 | size(8) = 44 | made(2) need(2) disk(4) cd_disk(4) | here(8) entries(8) cd_size(8) cd_off(8)
//   ZIP64 locator 50 4B 06 07 | disk(4) | end64_off(8) | disks(4)                                        (all little-endian)
//
// Sizes, CRC-32, method and flags of an entry always come from the directory (so entries written with a data descriptor,
// flag bit 3, need nothing special); the LOCAL header only says where the data starts: its own name and extra lengths
// legitimately differ from the directory's.  No alignment is assumed and every read is placed inside the bytes given before
// it happens.  Records are only ever reached from cd_off, so a signature inside a name, an extra field, a comment or an
// entry's data is never taken for a record.
// Out of scope: encryption, methods other than 0 and 8, multi-disk archives, archives with prepended data (the directory
// must end exactly where the end record starts), and a ZIP64 end record with an extensible data sector.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SF_ZIP_HD __host__ __device__ inline
#else
#define SF_ZIP_HD inline
#endif

namespace sf {
namespace zip {

constexpr uint32_t kLocal = 30, kCentral = 46, kEnd = 22, kEnd64 = 56, kLocator = 20;
constexpr uint32_t kMaxComment = 65535;
constexpr uint32_t kTail = kEnd + kMaxComment + kEnd64 + kLocator;  // the file's last bytes that can hold the end records
constexpr uint32_t kPiece = 32768;  // bytes of an entry's output per workgroup of the copy and per CRC-32 partial
// the reference's DecompressStatus values the parser produces, the per-entry code of an entry this library does not decode
// (SFH_ZIP_ENTRY_UNSUPPORTED: never a DecompressStatus), and read_index's return codes (SFH_OK, SFH_E_DST_TOO_SMALL)
constexpr uint32_t kStOk = 0, kStError = 1, kStDstTooSmall = 4, kStSrcTooSmall = 5, kEntryUnsupported = 0xFFFFFFF9u;
constexpr int kOk = 0, kDstTooSmall = -2;
constexpr uint32_t kFlagsRefused = 1u << 0 | 1u << 5 | 1u << 6 | 1u << 13;  // encryption, patch data, strong encryption, masked directory

SF_ZIP_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }  // (no alignment assumed)
SF_ZIP_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
SF_ZIP_HD uint64_t le64(const uint8_t* p) { return le32(p) | (uint64_t)le32(p + 4) << 32; }
SF_ZIP_HD void st16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}
SF_ZIP_HD void st32(uint8_t* p, uint32_t v) {
  st16(p, v);
  st16(p + 2, v >> 16);
}
SF_ZIP_HD void st64(uint8_t* p, uint64_t v) {
  st32(p, (uint32_t)v);
  st32(p + 4, (uint32_t)(v >> 32));
}
SF_ZIP_HD bool sig(const uint8_t* p, uint8_t a, uint8_t b) { return p[0] == 0x50 && p[1] == 0x4B && p[2] == a && p[3] == b; }
SF_ZIP_HD uint64_t round16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// ---- the end record ----
// The highest position q in the last min(n, 22 + 65535) bytes that holds 50 4B 05 06 and whose comment ends the file (q + 22 +
// comment_len == n): the choice unzip and zipfile make.  UINT64_MAX: none.
SF_ZIP_HD uint64_t find_eocd(const uint8_t* p, uint64_t n) {
  if (n < kEnd) return ~0ull;
  const uint64_t lo = n > kEnd + kMaxComment ? n - (kEnd + kMaxComment) : 0;
  for (uint64_t q = n - kEnd + 1; q-- > lo;)
    if (sig(p + q, 5, 6) && q + kEnd + le16(p + q + 20) == n) return q;
  return ~0ull;
}

struct End {
  uint64_t entries, cd_off, cd_size;
  uint32_t zip64, status;
};

// The end records of a file of n bytes, read from its last tail_n bytes at `tail` (tail_n = min(n, kTail) always suffices: the
// host passes the whole file, the device call copies the tail down).  Offsets in the records are the FILE's.
SF_ZIP_HD uint32_t read_end(const uint8_t* tail, uint64_t tail_n, uint64_t n, End& E) {
  E = End{0, 0, 0, 0, kStOk};
  if (n < kEnd || tail_n < kEnd) return E.status = n < kEnd ? kStSrcTooSmall : kStError;
  const uint64_t base = n - tail_n, q = find_eocd(tail, tail_n);
  if (q == ~0ull) return E.status = kStError;
  const uint8_t* e = tail + q;
  if (le16(e + 4) != 0 || le16(e + 6) != 0 || le16(e + 8) != le16(e + 10)) return E.status = kStError;  // multi-disk
  uint64_t entries = le16(e + 10), cd_size = le32(e + 12), cd_off = le32(e + 16), end_at = base + q;
  if (entries == 0xFFFFu || cd_size == 0xFFFFFFFFu || cd_off == 0xFFFFFFFFu) {
    // the locator stands right in front of the end record, the ZIP64 end record (no extensible data) right in front of it.
    // No locator: the classic values stand as they are (an archive of exactly 65535 entries), as zipfile reads them
    if (q >= kLocator && sig(e - kLocator, 6, 7)) {
      if (q < kEnd64 + kLocator) return E.status = kStError;
      const uint8_t* l = e - kLocator;
      const uint8_t* r = l - kEnd64;
      if (le32(l + 4) != 0 || le32(l + 16) > 1) return E.status = kStError;
      end_at -= kEnd64 + kLocator;
      if (le64(l + 8) != end_at || !sig(r, 6, 6) || le64(r + 4) != kEnd64 - 12) return E.status = kStError;
      if (le32(r + 16) != 0 || le32(r + 20) != 0 || le64(r + 24) != le64(r + 32)) return E.status = kStError;
      entries = le64(r + 32);
      cd_size = le64(r + 40);
      cd_off = le64(r + 48);
      E.zip64 = 1;
    }
  }
  // the directory ends exactly where the (ZIP64) end record starts, and holds at least 46 bytes per entry
  if (cd_off > end_at || cd_size != end_at - cd_off || entries > cd_size / kCentral) return E.status = kStError;
  E.entries = entries;
  E.cd_off = cd_off;
  E.cd_size = cd_size;
  return kStOk;
}

// ---- the entry table: sfh_zip_entry's layout ----
struct Entry {
  uint64_t local_off, data_off, csize, usize, out_off, name_off;
  uint32_t crc32, status;
  uint16_t method, flags, name_len, pad;
};
static_assert(sizeof(Entry) == 64, "sfh_zip_entry");

// The directory record at byte `at` of the cd_n directory bytes at cd (the directory starts at byte cd_off of the file, which
// only places name_off).  kStOk: E holds the directory's word on the entry (data_off 0, out_off 0; status: kEntryUnsupported
// for a method other than 0 and 8 or a refused flag, kStError for a stored entry with csize != usize, else 0) and *next = the
// next record.  kStError: no signature, the record or its name, extra field and comment reach past cd_n, a 0x0001 subfield
// that lacks a saturated value, or a subfield that overruns the extra field.
SF_ZIP_HD uint32_t parse_central(const uint8_t* cd, uint64_t cd_n, uint64_t at, uint64_t cd_off, Entry& E, uint64_t& next) {
  E = Entry{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  next = at;
  if (at > cd_n || cd_n - at < kCentral) return kStError;
  const uint8_t* r = cd + at;
  if (!sig(r, 1, 2)) return kStError;
  const uint32_t nlen = le16(r + 28), xlen = le16(r + 30), clen = le16(r + 32);
  if (cd_n - at - kCentral < (uint64_t)nlen + xlen + clen) return kStError;
  E.flags = (uint16_t)le16(r + 8);
  E.method = (uint16_t)le16(r + 10);
  E.crc32 = le32(r + 16);
  E.csize = le32(r + 20);
  E.usize = le32(r + 24);
  E.local_off = le32(r + 42);
  E.name_len = (uint16_t)nlen;
  E.name_off = cd_off + at + kCentral;
  const uint8_t* x = r + kCentral + nlen;
  for (uint32_t k = 0; xlen - k >= 4;) {  // (fewer than four bytes left over: padding, as zipfile reads it)
    const uint32_t id = le16(x + k), len = le16(x + k + 2);
    if (len > xlen - k - 4) return kStError;
    if (id == 0x0001) {  // the saturated values, in this order
      uint32_t u = 0;
      uint64_t* const slot[3] = {&E.usize, &E.csize, &E.local_off};
      for (uint32_t j = 0; j < 3; ++j) {
        if (*slot[j] != 0xFFFFFFFFu) continue;
        if (len - u < 8) return kStError;
        *slot[j] = le64(x + k + 4 + u);
        u += 8;
      }
    }
    k += 4 + len;
  }
  if ((E.method != 0 && E.method != 8) || (E.flags & kFlagsRefused)) E.status = kEntryUnsupported;
  else if (E.method == 0 && E.csize != E.usize) E.status = kStError;
  next = at + kCentral + nlen + xlen + clen;
  return kStOk;
}

// Record by record from the directory's first byte: exactly `entries` records that end exactly on cd_n.  out (nullable: the
// check alone) gets the entries, out_off the running sum of the sizes rounded up to 16 (entries with a status count too: the
// layout does not depend on what decodes); *total_out = that sum over all.
SF_ZIP_HD uint32_t walk_central(const uint8_t* cd, uint64_t cd_n, uint64_t cd_off, uint64_t entries, Entry* out, uint64_t* total_out) {
  uint64_t at = 0, o = 0;
  for (uint64_t i = 0; i < entries; ++i) {
    Entry E;
    uint64_t next;
    if (parse_central(cd, cd_n, at, cd_off, E, next) != kStOk) return kStError;
    E.out_off = o;
    if (E.usize > (1ull << 62)) return kStError;  // (no sum of sizes a file can state overflows below)
    o += round16(E.usize);
    if (o > (1ull << 63)) return kStError;
    if (out) out[i] = E;
    at = next;
  }
  if (at != cd_n) return kStError;
  *total_out = o;
  return kStOk;
}

// The local header of an entry the directory gave status 0, in the file's first `limit` bytes at p (limit = cd_off: entry data
// lies in front of the directory): data_off and the entry's status.  kStSrcTooSmall: the header or [data_off, data_off + csize)
// reaches past limit; kStError: no local signature.  An entry that already has a status keeps it and is not read.
SF_ZIP_HD uint32_t parse_local(const uint8_t* p, uint64_t limit, Entry& E) {
  if (E.status != kStOk) return E.status;
  if (E.local_off > limit || limit - E.local_off < kLocal) return E.status = kStSrcTooSmall;
  const uint8_t* h = p + E.local_off;
  if (!sig(h, 3, 4)) return E.status = kStError;
  const uint64_t data = E.local_off + kLocal + le16(h + 26) + le16(h + 28);
  if (data > limit || limit - data < E.csize) return E.status = kStSrcTooSmall;
  E.data_off = data;
  return kStOk;
}

struct Info {
  uint64_t entries, cd_off, cd_size, total_out;
  uint32_t zip64, status;
};

// The host's walk over a whole file.  Returns kDstTooSmall when cap < entries (I then holds the counts: what to allocate); the
// table is written only on kOk with status kStOk, and with another status the counts are 0.
inline int read_index(const uint8_t* p, uint64_t n, Info& I, Entry* out, uint64_t cap) {
  I = Info{0, 0, 0, 0, 0, kStOk};
  End E;
  if (read_end(p, n, n, E) != kStOk) {
    I.status = E.status;
    return kOk;
  }
  uint64_t total = 0;
  if (walk_central(p + E.cd_off, E.cd_size, E.cd_off, E.entries, nullptr, &total) != kStOk) {
    I.status = kStError;
    return kOk;
  }
  I = Info{E.entries, E.cd_off, E.cd_size, total, E.zip64, kStOk};
  if (cap < E.entries) return kDstTooSmall;
  walk_central(p + E.cd_off, E.cd_size, E.cd_off, E.entries, out, &total);
  for (uint64_t i = 0; i < E.entries; ++i) parse_local(p, E.cd_off, out[i]);
  return kOk;
}

// ---- the writer's arithmetic ----
// What the writer stores: deflated entries, UTF-8 names (flag bit 11), time 0 and date 1980-01-01 (deterministic, like gzip's
// MTIME 0), no extra fields, no comments, external attributes 0.
constexpr uint32_t kWriteFlags = 0x0800, kWriteMethod = 8, kWriteDate = 0x0021, kWriteNeed = 20, kWriteNeed64 = 45;
constexpr uint64_t kMaxItem = 0xFFFFFFFFull;  // an item of this many bytes or more needs ZIP64 sizes: refused by the writer

SF_ZIP_HD uint32_t write_local(uint8_t* d, const uint8_t* name, uint32_t name_len, uint32_t crc, uint32_t csize, uint32_t usize) {
  const uint8_t h[4] = {0x50, 0x4B, 3, 4};
  for (uint32_t k = 0; k < 4; ++k) d[k] = h[k];
  st16(d + 4, kWriteNeed);
  st16(d + 6, kWriteFlags);
  st16(d + 8, kWriteMethod);
  st16(d + 10, 0);
  st16(d + 12, kWriteDate);
  st32(d + 14, crc);
  st32(d + 18, csize);
  st32(d + 22, usize);
  st16(d + 26, name_len);
  st16(d + 28, 0);
  for (uint32_t k = 0; k < name_len; ++k) d[kLocal + k] = name[k];
  return kLocal + name_len;
}

SF_ZIP_HD uint32_t write_central(uint8_t* d, const uint8_t* name, uint32_t name_len, uint32_t crc, uint32_t csize, uint32_t usize,
                                 uint32_t local_off) {
  const uint8_t h[4] = {0x50, 0x4B, 1, 2};
  for (uint32_t k = 0; k < 4; ++k) d[k] = h[k];
  st16(d + 4, kWriteNeed);  // version made by: 2.0, host system 0
  st16(d + 6, kWriteNeed);
  st16(d + 8, kWriteFlags);
  st16(d + 10, kWriteMethod);
  st16(d + 12, 0);
  st16(d + 14, kWriteDate);
  st32(d + 16, crc);
  st32(d + 20, csize);
  st32(d + 24, usize);
  st16(d + 28, name_len);
  for (uint32_t k = 30; k < 42; ++k) d[k] = 0;  // extra, comment, disk, internal and external attributes
  st32(d + 42, local_off);
  for (uint32_t k = 0; k < name_len; ++k) d[kCentral + k] = name[k];
  return kCentral + name_len;
}

// bytes of the end record(s) for `entries` entries, and the records themselves at d: the classic one, and with more than
// 65535 entries the ZIP64 end record and its locator in front of it (the classic count saturated, as the specification says;
// the sizes and offsets the writer produces always fit 32 bits)
SF_ZIP_HD uint32_t end_bytes(uint64_t entries) { return entries > 0xFFFFu ? kEnd64 + kLocator + kEnd : kEnd; }
SF_ZIP_HD uint32_t write_end(uint8_t* d, uint64_t entries, uint64_t cd_off, uint64_t cd_size) {
  uint32_t at = 0;
  const bool z64 = entries > 0xFFFFu;
  if (z64) {
    const uint8_t h[4] = {0x50, 0x4B, 6, 6};
    for (uint32_t k = 0; k < 4; ++k) d[k] = h[k];
    st64(d + 4, kEnd64 - 12);
    st16(d + 12, kWriteNeed64);
    st16(d + 14, kWriteNeed64);
    st32(d + 16, 0);
    st32(d + 20, 0);
    st64(d + 24, entries);
    st64(d + 32, entries);
    st64(d + 40, cd_size);
    st64(d + 48, cd_off);
    uint8_t* l = d + kEnd64;
    const uint8_t g[4] = {0x50, 0x4B, 6, 7};
    for (uint32_t k = 0; k < 4; ++k) l[k] = g[k];
    st32(l + 4, 0);
    st64(l + 8, cd_off + cd_size);
    st32(l + 16, 1);
    at = kEnd64 + kLocator;
  }
  uint8_t* e = d + at;
  const uint8_t h[4] = {0x50, 0x4B, 5, 6};
  for (uint32_t k = 0; k < 4; ++k) e[k] = h[k];
  st16(e + 4, 0);
  st16(e + 6, 0);
  st16(e + 8, z64 ? 0xFFFFu : (uint32_t)entries);
  st16(e + 10, z64 ? 0xFFFFu : (uint32_t)entries);
  st32(e + 12, (uint32_t)cd_size);
  st32(e + 16, (uint32_t)cd_off);
  st16(e + 20, 0);
  return at + kEnd;
}

// sfh_compress_bound(n, 0), restated (the bound is per 32 KiB block), and sfh_zip_bound: every item's local header, name and
// bound, the directory, and the end records.  0: the sum overflows.
SF_ZIP_HD uint64_t body_bound(uint64_t n) { return (n ? (n + 32767) / 32768 : 1) * (uint64_t)(32768 + 32768 / 8 + 640); }
SF_ZIP_HD uint64_t bound(uint64_t count, const uint64_t* src_n, const uint32_t* name_len) {
  uint64_t b = kEnd + kEnd64 + kLocator;
  for (uint64_t i = 0; i < count; ++i) {
    if (src_n[i] > (1ull << 44)) return 0;
    b += kLocal + kCentral + 2ull * name_len[i] + body_bound(src_n[i]);
    if (b > (1ull << 62)) return 0;
  }
  return b;
}

}  // namespace zip
}  // namespace sf
