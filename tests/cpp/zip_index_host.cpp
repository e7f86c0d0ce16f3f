// The ZIP plan (starflate_amd/csrc/sf_zip_plan.h) compiled for the host: as a shared library for tests/test_zip_index_host.py
// (-Wall -Wextra -Werror), and as a stand-alone program under AddressSanitizer + UBSan.  The program reads cases from a file
// (u64 size, then the bytes), puts every archive into a heap block of exactly its size and prints one digest of the index per
// case; `sweep` runs every truncation of the first case and three corruptions of every byte of its directory and end records
// and prints one digest over all of them.  A read outside an archive is a sanitizer report there.
#include "../../starflate_amd/csrc/sf_zip_plan.h"

#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>

namespace z = sf::zip;

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}

// the index of n bytes at p, twice as a caller runs it (the counts, then the table), folded into one number
static uint64_t digest(const uint8_t* p, uint64_t n) {
  z::Info I;
  int rc = z::read_index(p, n, I, nullptr, 0);
  uint64_t h = 0xCBF29CE484222325ull;
  h = fnv(h, &rc, sizeof rc);
  h = fnv(h, &I, sizeof I);
  if (I.status != z::kStOk || I.entries == 0) return h;
  std::unique_ptr<z::Entry[]> E(new z::Entry[I.entries]);
  rc = z::read_index(p, n, I, E.get(), I.entries);
  h = fnv(h, &rc, sizeof rc);
  for (uint64_t i = 0; i < I.entries; ++i) {
    h = fnv(h, &E[i], sizeof(z::Entry));
    if (E[i].name_off + E[i].name_len <= n) h = fnv(h, p + E[i].name_off, E[i].name_len);  // (the names, where the table says)
  }
  return h;
}

extern "C" {
uint64_t sfz_digest(const uint8_t* p, uint64_t n) { return digest(p, n); }
int sfz_read_index(const uint8_t* p, uint64_t n, z::Info* info, z::Entry* entries, uint64_t cap) {
  return z::read_index(p, n, *info, entries, cap);
}
uint64_t sfz_find_eocd(const uint8_t* p, uint64_t n) { return z::find_eocd(p, n); }
uint32_t sfz_write_local(uint8_t* d, const uint8_t* name, uint32_t nlen, uint32_t crc, uint32_t csize, uint32_t usize) {
  return z::write_local(d, name, nlen, crc, csize, usize);
}
uint32_t sfz_write_central(uint8_t* d, const uint8_t* name, uint32_t nlen, uint32_t crc, uint32_t csize, uint32_t usize, uint32_t off) {
  return z::write_central(d, name, nlen, crc, csize, usize, off);
}
uint32_t sfz_end_bytes(uint64_t entries) { return z::end_bytes(entries); }
uint32_t sfz_write_end(uint8_t* d, uint64_t entries, uint64_t cd_off, uint64_t cd_size) { return z::write_end(d, entries, cd_off, cd_size); }
uint64_t sfz_bound(uint64_t count, const uint64_t* src_n, const uint32_t* name_len) { return z::bound(count, src_n, name_len); }
}

// a copy of n bytes in a heap block of exactly n bytes
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, uint64_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
  if (n) memcpy(b.get(), p, n);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<std::vector<uint8_t>> cases;
  for (uint64_t n; fread(&n, 8, 1, f) == 1;) {
    std::vector<uint8_t> b(n);
    if (n && fread(b.data(), 1, n, f) != n) return 2;
    cases.push_back(std::move(b));
  }
  fclose(f);
  for (const auto& c : cases) printf("%llu\n", (unsigned long long)digest(exact(c.data(), c.size()).get(), c.size()));
  if (argc > 2 && !strcmp(argv[2], "sweep") && !cases.empty()) {
    const auto& c = cases[0];
    z::Info I;
    z::read_index(c.data(), c.size(), I, nullptr, 0);
    uint64_t h = 0;
    for (uint64_t n = 0; n < c.size(); ++n) h = fnv(h ^ digest(exact(c.data(), n).get(), n), &n, 8);
    const uint8_t flips[3] = {0x01, 0x80, 0xFF};
    for (uint64_t at = I.cd_off; at < c.size(); ++at)
      for (uint8_t x : flips) {
        auto b = exact(c.data(), c.size());
        b[at] ^= x;
        h = fnv(h ^ digest(b.get(), c.size()), &at, 8);
      }
    printf("sweep %llu\n", (unsigned long long)h);
  }
  printf("%zu cases\n", cases.size());
  return 0;
}
