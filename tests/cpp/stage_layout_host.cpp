// Host shim for tests/test_stage_layout_host.py: where the batched host-buffer entry points put their items -- the packed
// layout of sf_stage_plan.h, and the piece of the stream a decode span of sfh_decompress_ranges uploads (sf_range_plan.h).
// TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_range_plan.h"
#include "../../starflate_amd/csrc/sf_stage_plan.h"

extern "C" {

// off[0 .. count] of `count` slot sizes
void sfl_pack_layout(const uint64_t* slot, uint64_t count, uint64_t* off) { sf::stage::pack_layout(slot, (size_t)count, off); }

// the piece of a span of `nrows` rows from segment `first_seg` on -> out[0] = lo, out[1] = n
void sfl_source_piece(uint64_t first_seg, uint32_t nrows, const uint64_t* index, uint64_t src_n, uint64_t* out) {
  const sf::range::Piece p = sf::range::source_piece(sf::range::Span{first_seg, 0, nrows}, index, src_n);
  out[0] = p.lo;
  out[1] = p.n;
}
}
