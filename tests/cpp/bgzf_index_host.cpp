// The BGZF member parser (starflate_amd/csrc/sf_bgzf_plan.h) compiled for the host: tests/test_bgzf_host.py compares what it
// reads from files made with Python's zlib with a pure-Python walker, through sfbgzf_read (a shared library), and runs the
// same cases through main() below, built with AddressSanitizer + UBSan: every case in a heap allocation of exactly its size,
// its arrays of exactly members + 1 entries, so a read past src_n or a store past the arrays is a report.
#include "../../starflate_amd/csrc/sf_bgzf_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" {

// out[0..5] = rc, status, members, max_isize, has_eof, total_n
void sfbgzf_read(const uint8_t* src, uint64_t n, uint64_t* member_off, uint64_t* out_off, uint64_t cap, int64_t* out) {
  sf::bgzf::Info I;
  const int rc = sf::bgzf::read_index(src, n, I, member_off, out_off, cap);
  out[0] = rc;
  out[1] = I.status;
  out[2] = I.members;
  out[3] = I.max_isize;
  out[4] = I.has_eof;
  out[5] = (int64_t)I.total_n;
}

uint64_t sfbgzf_bound(uint64_t n) { return sf::bgzf::bound(n); }

}  // extern "C"

// main(cases file): the file holds case after case, each a u64 little-endian length and that many bytes.  Prints one line per
// case: rc status members max_isize has_eof total_n and a sum over both arrays.
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  size_t cases = 0;
  for (;;) {
    uint64_t n = 0;
    if (fread(&n, sizeof n, 1, f) != 1) break;
    uint8_t* p = (uint8_t*)malloc(n ? (size_t)n : 1);  // exactly the case's bytes
    if (!p || (n && fread(p, 1, (size_t)n, f) != n)) return 2;
    sf::bgzf::Info I;
    int rc = sf::bgzf::read_index(p, n, I, nullptr, nullptr, 0);  // the count: one entry is needed at least
    uint64_t sum = 0;
    if (I.status == sf::bgzf::kStOk) {
      if (rc != sf::bgzf::kDstTooSmall) return 3;
      std::vector<uint64_t> less(I.members), a((size_t)I.members + 1), b((size_t)I.members + 1);  // exactly the entries
      sf::bgzf::Info J;
      if (sf::bgzf::read_index(p, n, J, less.data(), less.data(), less.size()) != sf::bgzf::kDstTooSmall) return 3;
      rc = sf::bgzf::read_index(p, n, I, a.data(), b.data(), a.size());
      if (rc != sf::bgzf::kOk) return 3;
      for (uint64_t v : a) sum += v;
      for (uint64_t v : b) sum += v;
    }
    printf("%d %u %u %u %u %llu %llu\n", rc, I.status, I.members, I.max_isize, I.has_eof, (unsigned long long)I.total_n,
           (unsigned long long)sum);
    free(p);
    ++cases;
  }
  fclose(f);
  printf("%zu cases\n", cases);
  return 0;
}
