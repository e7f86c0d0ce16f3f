// Host side of the multi-member gzip tests (tests/test_stream_members_host.py, tests/test_gpu_stream_members.py): the
// specification, container.hpp's decompress_members(), behind a C ABI, and the steps the device runs between two members
// (starflate_amd/csrc/sf_members.h: header_end, hop, head_candidate) walked over the same bytes and compared with it.
// With -DSFM_MAIN a stand-alone program for the sanitizers: sfm_agree on every prefix of the file named on its command line.
// TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_members.h"
#include "starflate/container.hpp"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <span>
#include <vector>

namespace {

std::span<const std::byte> bytes(const uint8_t* p, uint64_t n) { return {reinterpret_cast<const std::byte*>(p), static_cast<std::size_t>(n)}; }

}  // namespace

extern "C" {

// decompress_members(src, dst[cap]) -> its status; *produced (Success only); the members that passed into recs[0, rec_cap) as
// {u64 src_end, u64 out_end, u32 crc32, u32 isize}, *nrec: how many there were
uint32_t sfm_members(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, uint64_t* produced, starflate::GzipMember* recs,
                     uint64_t rec_cap, uint64_t* nrec) {
  std::vector<starflate::GzipMember> m;
  std::size_t out = 0;
  const auto st = starflate::decompress_members(bytes(src, n), {reinterpret_cast<std::byte*>(dst), static_cast<std::size_t>(cap)}, &out, &m);
  *produced = out;
  *nrec = m.size();
  for (uint64_t i = 0; i < m.size() && i < rec_cap; ++i) recs[i] = m[i];
  return static_cast<uint32_t>(st);
}

// The file again with sf_members.h between the bodies (the raw decoder finds each body's end), into a dst of `cap` bytes:
// 0 when status, member rows and head positions agree with the specification, else the line of the first difference.
int sfm_agree(const uint8_t* src, uint64_t n, uint64_t cap) {
  std::vector<std::byte> d0(cap), d1(cap);
  std::vector<starflate::GzipMember> want, got;
  std::size_t out0 = 0;
  const auto spec = static_cast<uint32_t>(starflate::decompress_members(bytes(src, n), d0, &out0, &want));
  uint32_t st = 0;
  uint64_t out = 0, head = 0;
  if (n == 0) {
    st = sf::members::kStSrcTooSmall;  // (header_end takes at <= n: the same answer, but nothing to point at)
  } else {
    uint64_t body = sf::members::header_end(src, 0, n, st);
    while (st == 0) {
      if (!sf::members::head_candidate(src, head, n)) return __LINE__;
      std::ptrdiff_t w = 0;
      std::size_t used = 0;
      st = static_cast<uint32_t>(starflate::decompress(bytes(src + body, n - body), std::span<std::byte>{d1}.subspan(out), &w, &used));
      if (st) break;
      const sf::members::Hop h = sf::members::hop(src, n, 8 * (body + used));
      if (h.st && h.src_end == 0) {  // no trailer
        st = h.st;
        break;
      }
      const auto own = std::span<const std::byte>{d1}.subspan(out, static_cast<std::size_t>(w));
      if (h.isize != static_cast<uint32_t>(w) || h.crc32 != starflate::crc32(own)) {
        st = sf::members::kStError;
        break;
      }
      out += static_cast<uint64_t>(w);
      got.push_back({h.src_end, out, h.crc32, h.isize});
      if (h.end) break;
      st = h.st;
      head = h.src_end;
      while (src[head] == 0) ++head;
      body = h.next;
    }
  }
  if (st != spec) return __LINE__;
  if (got.size() != want.size()) return __LINE__;
  for (std::size_t i = 0; i < got.size(); ++i)
    if (got[i].src_end != want[i].src_end || got[i].out_end != want[i].out_end || got[i].crc32 != want[i].crc32 ||
        got[i].isize != want[i].isize)
      return __LINE__;
  if (st == 0 && (out != out0 || !std::equal(d0.begin(), d0.begin() + static_cast<std::ptrdiff_t>(out), d1.begin()))) return __LINE__;
  return 0;
}

// every byte position in [lo, hi) of src[0, n) where head_candidate holds -> hits[0, cap); returns the count
uint64_t sfm_head_candidates(const uint8_t* src, uint64_t n, uint64_t lo, uint64_t hi, uint64_t* hits, uint64_t cap) {
  uint64_t k = 0;
  for (uint64_t at = lo; at < hi && at < n; ++at)
    if (sf::members::head_candidate(src, at, n)) {
      if (k < cap) hits[k] = at;
      ++k;
    }
  return k;
}
}

#ifdef SFM_MAIN
// usage: members_host FILE CAP -- every prefix of FILE (each in a buffer of exactly its length, so that a read past n is the
// sanitizer's to report) through sfm_agree and sfm_head_candidates
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  for (int c; (c = std::fgetc(f)) != EOF;) file.push_back(static_cast<uint8_t>(c));
  std::fclose(f);
  const uint64_t cap = std::strtoull(argv[2], nullptr, 10);
  for (std::size_t n = 0; n <= file.size(); ++n) {
    const std::vector<uint8_t> prefix(file.begin(), file.begin() + static_cast<std::ptrdiff_t>(n));
    if (const int line = sfm_agree(prefix.data(), n, cap)) {
      std::printf("prefix %zu: disagreement at line %d\n", n, line);
      return 1;
    }
    uint64_t hit = 0;
    sfm_head_candidates(prefix.data(), n, 0, n, &hit, 1);
  }
  std::printf("%zu prefixes agree\n", file.size() + 1);
  return 0;
}
#endif
