// Host side of the stream decoder's tests (tests/test_stream_find_host.py, tests/test_stream_chain.py, tests/test_gpu_stream.py):
// the block-start predicate of sf_inflate_core.h and the chain round of sf_stream_chain.h compiled for the host, and container.hpp's serial decoder behind a C ABI (the status every GPU result is
// compared with).  TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_inflate_core.h"
#include "../../starflate_amd/csrc/sf_stream_chain.h"
#include "starflate/container.hpp"

#include <cstddef>
#include <cstdint>
#include <span>
#include <vector>

extern "C" {

// every bit offset p in [lo, hi) of buf[0, n) where dynamic_header_candidate holds -> hits[0, cap); returns the count (buf is
// readable up to the next multiple of 4 bytes)
uint64_t sfs_scan(const uint8_t* buf, uint64_t n, uint64_t lo, uint64_t hi, uint64_t* hits, uint64_t cap) {
  uint64_t k = 0;
  uint8_t lut[128];
  for (uint64_t p = lo; p < hi && p < 8 * n; ++p) {
    sf::inflate::BitReader br;
    br.open(buf, n, p >> 3, n);
    br.refill();
    br.drop(static_cast<uint32_t>(p & 7));
    if (sf::inflate::dynamic_header_candidate(br, lut)) {
      if (k < cap) hits[k] = p;
      ++k;
    }
  }
  return k;
}

// container.hpp's decompress(src, dst, container) for a dst of `cap` bytes -> its status; *produced: the body's bytes
// (raw and gzip; zlib: -1)
uint32_t sfs_serial(const uint8_t* src, uint64_t n, uint32_t container, uint8_t* dst, uint64_t cap, int64_t* produced) {
  const std::span<const std::byte> s{reinterpret_cast<const std::byte*>(src), static_cast<std::size_t>(n)};
  const std::span<std::byte> d{reinterpret_cast<std::byte*>(dst), static_cast<std::size_t>(cap)};
  *produced = -1;
  if (container == 0) {
    std::ptrdiff_t w = 0;
    const auto st = starflate::decompress(s, d, &w);
    *produced = w;
    return static_cast<uint32_t>(st);
  }
  return static_cast<uint32_t>(starflate::decompress(s, d, container == 1 ? starflate::Container::Zlib : starflate::Container::Gzip));
}

// sf::stream_chain_round over rec[0, m) (updated in place) -> the chunks to decode again in redo[0, return); *chain
uint32_t sfs_chain_round(sf::StreamChunk* rec, uint32_t m, uint32_t* redo, uint32_t* chain) {
  std::vector<uint32_t> r;
  sf::stream_chain_round(rec, 0, m, r, chain);
  for (size_t i = 0; i < r.size(); ++i) redo[i] = r[i];
  return static_cast<uint32_t>(r.size());
}
}
