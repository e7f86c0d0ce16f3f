// The dictzip table parser (starflate_amd/csrc/sf_dz_plan.h) compiled for the host: tests/test_dictzip_host.py compares what
// it reads from files made by a Python dictzip writer with that writer's own offsets, through sfdz_read (a shared library),
// and runs the same cases through main() below, built with AddressSanitizer + UBSan: every case in a heap allocation of
// exactly its size, its index in one of exactly nseg + 1 entries, so a read past src_n or a store past the index is a report.
#include "../../starflate_amd/csrc/sf_dz_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" {

// out[0..4] = rc, status, nseg, header_bytes, total_n (the last four 0 unless rc == 0; all but status 0 unless status == 0)
void sfdz_read(const uint8_t* src, uint64_t n, uint64_t* index, uint64_t index_cap, int64_t* out) {
  sf::dz::Head H;
  const int rc = sf::dz::read_index(src, n, H, index, index_cap);
  const bool parsed = rc == sf::dz::kOk, ok = parsed && H.status == sf::dz::kStOk;
  out[0] = rc;
  out[1] = parsed ? H.status : 0;
  out[2] = ok ? H.nseg : 0;
  out[3] = ok ? H.header_bytes : 0;
  out[4] = ok ? (int64_t)H.total_n : 0;
}

uint64_t sfdz_header_bytes(uint64_t n) { return sf::dz::header_bytes(n); }

}  // extern "C"

// main(cases file): the file holds case after case, each a u64 little-endian length and that many bytes.  Prints one line per
// case: rc status nseg header_bytes total_n and a sum over the index entries.
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
    sf::dz::Head H;
    int rc = sf::dz::parse_head(p, n, H);
    uint64_t sum = 0;
    if (rc == sf::dz::kOk && H.status == sf::dz::kStOk) {
      std::vector<uint64_t> index((size_t)H.nseg + 1);  // exactly the entries the index takes
      rc = sf::dz::read_index(p, n, H, index.data(), index.size());
      if (rc == sf::dz::kOk && H.status == sf::dz::kStOk)
        for (uint64_t v : index) sum += v;
      // one entry short: refused, nothing stored
      std::vector<uint64_t> less((size_t)H.nseg);
      sf::dz::Head H2;
      if (H.status == sf::dz::kStOk && sf::dz::read_index(p, n, H2, less.data(), less.size()) != sf::dz::kDstTooSmall) return 3;
    }
    const bool ok = rc == sf::dz::kOk && H.status == sf::dz::kStOk;
    printf("%d %u %u %u %llu %llu\n", rc, rc == sf::dz::kOk ? H.status : 0u, ok ? H.nseg : 0u, ok ? H.header_bytes : 0u,
           ok ? (unsigned long long)H.total_n : 0ull, (unsigned long long)sum);
    free(p);
    ++cases;
  }
  fclose(f);
  printf("%zu cases\n", cases);
  return 0;
}
