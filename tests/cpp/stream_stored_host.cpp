// Host side of tests/test_stream_stored_find_host.py: the stored-block start predicate of sf_inflate_core.h compiled for the
// host, read through a BitReader opened as k_stream_find opens it.  TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_inflate_core.h"

#include <cstdint>

extern "C" {

// every bit offset p in [lo, hi) of the body buf[0, n) where stored_header_candidate holds -> hits[0, cap); returns the count
// (buf is readable up to the next multiple of 4 bytes).  min_len, look: what k_stream_find asks of a hit besides (0, 0: the
// predicate alone): LEN >= min_len (0 in the library), and stored_run_follows behind the payload
uint64_t sfss_scan(const uint8_t* buf, uint64_t n, uint64_t lo, uint64_t hi, uint64_t* hits, uint64_t cap, uint32_t min_len,
                   uint32_t look) {
  uint64_t k = 0;
  for (uint64_t p = lo; p < hi && p < 8 * n; ++p) {
    sf::inflate::BitReader br;
    br.open(buf, n, p >> 3, n);
    br.refill();
    if (sf::inflate::stored_header_candidate(br, static_cast<uint32_t>(p & 7), p >> 3, n) &&
        sf::inflate::stored_header_len(br) >= min_len &&
        (!look || sf::inflate::stored_run_follows(buf, n, (p >> 3) + 5 + sf::inflate::stored_header_len(br)))) {
      if (k < cap) hits[k] = p;
      ++k;
    }
  }
  return k;
}
}
