// The BGZF random-access planner (starflate_amd/csrc/sf_bgzf_range_plan.h) compiled for the host: a shared library for
// tests/test_bgzf_range_plan_host.py (span_of, row_of, the batch cut and the virtual offsets one call at a time, against the
// test's brute-force model), and a stand-alone program -- built with AddressSanitizer + UBSan by the same test -- that runs
// the same enumeration over every list of member sizes in a case file, each index in a heap allocation of exactly its
// members + 1 entries, and prints one digest per list: the test holds them against sfbr_digest's.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../starflate_amd/csrc/sf_bgzf_range_plan.h"

namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(uint64_t v) {
    for (int k = 0; k < 8; ++k) {
      h ^= (v >> (8 * k)) & 0xFF;
      h *= 1099511628211ull;
    }
  }
};

// every offset within one byte of a member boundary; every length of {0, 1, 3, 4, 5, the remainder} that fits; batch_chunks
// 1, 2, 3 on narrow and on wide rows
uint64_t digest(const uint64_t* sizes, uint32_t members) {
  uint64_t* out_off = new uint64_t[(size_t)members + 1];
  uint64_t* member_off = new uint64_t[(size_t)members + 1];
  out_off[0] = member_off[0] = 0;
  for (uint32_t i = 0; i < members; ++i) {
    out_off[i + 1] = out_off[i] + sizes[i];
    member_off[i + 1] = member_off[i] + 26 + sizes[i] / 3;  // (any ascending file offsets)
  }
  const uint64_t total = out_off[members];
  Fnv F;
  std::vector<uint64_t> offs;
  for (uint32_t i = 0; i <= members; ++i)
    for (int d = -1; d <= 1; ++d) {
      const uint64_t o = out_off[i] + (uint64_t)(int64_t)d;
      if (o <= total) offs.push_back(o);  // (-1 at 0 wraps above total)
    }
  for (uint64_t off : offs) {
    const uint64_t lens[6] = {0, 1, 3, 4, 5, total - off};
    for (uint64_t len : lens) {
      if (len > total - off) continue;
      const sf::bgzf::Span S = sf::bgzf::span_of(out_off, members, off, len);
      F.add(S.first);
      F.add(S.rows);
      F.add(sf::bgzf::range_inside(out_off, members, off, len));
      const sf::bgzf::RangePiece P = sf::bgzf::range_piece(member_off, S, member_off[members]);
      F.add(P.lo);
      F.add(P.n);
      for (uint32_t k = 0; k < S.rows; ++k) {
        const sf::bgzf::RangeRow W = sf::bgzf::row_of(out_off, S.first, k, off, len);
        F.add(W.member);
        F.add(W.out_n);
        F.add(W.lo);
        F.add(W.hi);
        F.add(W.dst_off);
      }
      for (uint32_t bc = 1; bc <= 3; ++bc)
        for (int wide = 0; wide < 2; ++wide) {
          const uint32_t per = sf::bgzf::rows_per_batch(bc, wide != 0);
          const uint64_t nb = sf::bgzf::range_batches(S.rows, per);
          F.add(per);
          F.add(nb);
          for (uint64_t b = 0; b < nb; ++b) F.add(sf::bgzf::range_batch_rows(S.rows, per, b));
        }
    }
    const uint64_t v = sf::bgzf::offset_to_voffset(member_off, out_off, members, off);
    F.add(v);
    F.add(sf::bgzf::voffset_to_offset(member_off, out_off, members, v));
    F.add(sf::bgzf::voffset_to_offset(member_off, out_off, members, v + (1ull << 16)));
  }
  F.add(sf::bgzf::span_of(out_off, members, total, 1).rows);  // behind the output
  F.add(sf::bgzf::offset_to_voffset(member_off, out_off, members, total + 1));
  delete[] out_off;
  delete[] member_off;
  return F.h;
}

}  // namespace

extern "C" {

uint64_t sfbr_digest(const uint64_t* sizes, uint32_t members) { return digest(sizes, members); }

// out[0..2] = first, rows, range_inside
void sfbr_span(const uint64_t* out_off, uint32_t members, uint64_t off, uint64_t len, uint64_t* out) {
  const sf::bgzf::Span S = sf::bgzf::span_of(out_off, members, off, len);
  out[0] = S.first;
  out[1] = S.rows;
  out[2] = sf::bgzf::range_inside(out_off, members, off, len);
}

// out[0..4] = member, out_n, lo, hi, dst_off
void sfbr_row(const uint64_t* out_off, uint32_t first, uint32_t k, uint64_t off, uint64_t len, uint64_t* out) {
  const sf::bgzf::RangeRow W = sf::bgzf::row_of(out_off, first, k, off, len);
  out[0] = W.member;
  out[1] = W.out_n;
  out[2] = W.lo;
  out[3] = W.hi;
  out[4] = W.dst_off;
}

// out[0] = rows per batch, out[1] = batches, out[2 ..] = every batch's rows (cap entries at most)
void sfbr_batches(uint64_t rows, uint32_t batch_chunks, int wide, uint64_t* out, uint64_t cap) {
  const uint32_t per = sf::bgzf::rows_per_batch(batch_chunks, wide != 0);
  out[0] = per;
  out[1] = sf::bgzf::range_batches(rows, per);
  for (uint64_t b = 0; b < out[1] && b < cap; ++b) out[2 + b] = sf::bgzf::range_batch_rows(rows, per, b);
}

// out[0..1] = lo, n
void sfbr_piece(const uint64_t* member_off, uint32_t first, uint32_t rows, uint64_t src_n, uint64_t* out) {
  const sf::bgzf::RangePiece P = sf::bgzf::range_piece(member_off, sf::bgzf::Span{first, rows}, src_n);
  out[0] = P.lo;
  out[1] = P.n;
}

}  // extern "C"

// cases file: per list a u64 count, then its sizes (u64 each)
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t lists = 0, m = 0;
  while (fread(&m, sizeof m, 1, f) == 1) {
    std::vector<uint64_t> sizes((size_t)m);
    if (m && fread(sizes.data(), sizeof(uint64_t), (size_t)m, f) != m) return 3;
    printf("%llu\n", (unsigned long long)digest(sizes.data(), (uint32_t)m));
    ++lists;
  }
  fclose(f);
  printf("%llu lists\n", (unsigned long long)lists);
  return 0;
}
