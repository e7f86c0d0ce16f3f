// The indexed decoder's cut into launch batches (starflate_amd/csrc/sf_inflate_plan.h) compiled for the host:
// tests/test_inflate_plan_host.py checks what it plans, expanded by for_rows() as the library expands it, against a model.
#include "../../starflate_amd/csrc/sf_inflate_plan.h"

namespace {
sf::iplan::Plan g_plan;
}

extern "C" {

// counts[0..3] = segments, strips, batches, segments of the widest batch
void sfi_plan(size_t count, const uint64_t* dst_n, const uint32_t* block_bytes, uint32_t cap, uint64_t* counts) {
  sf::iplan::plan_batches(count, dst_n, block_bytes, cap, g_plan);
  counts[0] = g_plan.nseg;
  counts[1] = g_plan.nstrips;
  counts[2] = g_plan.batches.size();
  counts[3] = g_plan.widest;
}

// the tables as the library fills them -- rows: 4 uint64 each {item, segment of the item, out_n, hist}; strips: 2 each {first row
// counted from its batch's first, rows}; batches: 6 each {row0, nseg, strip0, nstrips, item0, k0}.  Returns rows written.
uint64_t sfi_read(const uint64_t* dst_n, const uint32_t* block_bytes, uint64_t* rows, uint64_t* strips, uint64_t* batches) {
  uint64_t g = 0, t = 0;
  for (size_t b = 0; b < g_plan.batches.size(); ++b) {
    const sf::iplan::Batch& B = g_plan.batches[b];
    const uint64_t v[6] = {B.row0, B.nseg, B.strip0, B.nstrips, B.item0, B.k0};
    for (int k = 0; k < 6; ++k) batches[6 * b + k] = v[k];
    sf::iplan::for_rows(
        B, dst_n, block_bytes,
        [&](uint32_t first, uint32_t n) {
          strips[2 * t] = first;
          strips[2 * t + 1] = n;
          ++t;
        },
        [&](size_t i, uint32_t k) {
          rows[4 * g] = i;
          rows[4 * g + 1] = k;
          rows[4 * g + 2] = sf::iplan::seg_out_n(dst_n[i], k);
          rows[4 * g + 3] = sf::iplan::seg_hist(k, sf::iplan::sps_of(block_bytes, i));
          ++g;
        });
  }
  return g;
}

}  // extern "C"
