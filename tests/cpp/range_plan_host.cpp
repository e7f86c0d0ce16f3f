// The random-access planner (starflate_amd/csrc/sf_range_plan.h) compiled for the host: tests/test_range_plan_host.py
// compares what it plans with a brute-force model.
#include "../../starflate_amd/csrc/sf_range_plan.h"

namespace {
sf::range::Plan g_plan;
}

extern "C" {

// counts[0..3] = rows, spans, strips, batches; counts[4] = rows of the widest batch
int sfr_plan(uint64_t total_n, uint32_t block_bytes, size_t count, const uint64_t* offsets, const uint64_t* lengths, uint32_t cap,
             uint64_t* counts) {
  const int rc = sf::range::plan_ranges(total_n, block_bytes, count, offsets, lengths, cap, g_plan);
  counts[0] = g_plan.rows.size();
  counts[1] = g_plan.spans.size();
  counts[2] = g_plan.strips.size();
  counts[3] = g_plan.batches.size();
  counts[4] = g_plan.widest;
  return rc;
}

// rows: 7 uint64 each {seg, dst_off, range, out_n, hist, lo, hi}; spans: 3 each {first_seg, row0, nrows}; strips: 2 each
// {row0 in its batch, nrows}; batches: 4 each {row0, nrows, strip0, nstrips}
void sfr_read(uint64_t* rows, uint64_t* spans, uint64_t* strips, uint64_t* batches) {
  for (size_t i = 0; i < g_plan.rows.size(); ++i) {
    const sf::range::Row& w = g_plan.rows[i];
    const uint64_t v[7] = {w.seg, w.dst_off, w.range, w.out_n, w.hist, w.lo, w.hi};
    for (int k = 0; k < 7; ++k) rows[7 * i + k] = v[k];
  }
  for (size_t i = 0; i < g_plan.spans.size(); ++i) {
    spans[3 * i] = g_plan.spans[i].first_seg;
    spans[3 * i + 1] = g_plan.spans[i].row0;
    spans[3 * i + 2] = g_plan.spans[i].nrows;
  }
  for (size_t i = 0; i < g_plan.strips.size(); ++i) {
    strips[2 * i] = g_plan.strips[i].row0;
    strips[2 * i + 1] = g_plan.strips[i].nrows;
  }
  for (size_t i = 0; i < g_plan.batches.size(); ++i) {
    batches[4 * i] = g_plan.batches[i].row0;
    batches[4 * i + 1] = g_plan.batches[i].nrows;
    batches[4 * i + 2] = g_plan.batches[i].strip0;
    batches[4 * i + 3] = g_plan.batches[i].nstrips;
  }
}

}  // extern "C"
