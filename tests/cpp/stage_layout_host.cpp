// Host shim for tests/test_stage_layout_host.py: where the batched host-buffer entry points put their items -- the packed
// layout of sf_stage_plan.h, and the piece of the stream a decode span of sfh_decompress_ranges uploads (sf_range_plan.h) --
// and how the C-ABI lays several arrays out in one scratch buffer (sf_stage_plan.h: Carve).
// TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_range_plan.h"
#include "../../starflate_amd/csrc/sf_stage_plan.h"
#include "../../starflate_amd/csrc/sf_stream_chain.h"

extern "C" {

// off[0 .. count] of `count` slot sizes
void sfl_pack_layout(const uint64_t* slot, uint64_t count, uint64_t* off) { sf::stage::pack_layout(slot, (size_t)count, off); }

// the piece of a span of `nrows` rows from segment `first_seg` on -> out[0] = lo, out[1] = n
void sfl_source_piece(uint64_t first_seg, uint32_t nrows, const uint64_t* index, uint64_t src_n, uint64_t* out) {
  const sf::range::Piece p = sf::range::source_piece(sf::range::Span{first_seg, 0, nrows}, index, src_n);
  out[0] = p.lo;
  out[1] = p.n;
}

// Carve: `n` pieces, piece k of count[k] elements of esize[k] bytes (1, 2, 4, 8, 12 or 72: one type each) -> off[k]; returns
// bytes(), or ~0 for a size without a type here
struct SflE12 {
  uint32_t w[3];
};
struct SflE72 {
  uint64_t w[9];
};
uint64_t sfl_carve(const uint32_t* esize, const uint64_t* count, uint64_t n, uint64_t* off) {
  sf::stage::Carve L;
  for (uint64_t k = 0; k < n; ++k) {
    const size_t c = (size_t)count[k];
    switch (esize[k]) {
      case 1: off[k] = L.add<uint8_t>(c); break;
      case 2: off[k] = L.add<uint16_t>(c); break;
      case 4: off[k] = L.add<uint32_t>(c); break;
      case 8: off[k] = L.add<uint64_t>(c); break;
      case 12: off[k] = L.add<SflE12>(c); break;
      case 72: off[k] = L.add<SflE72>(c); break;
      default: return ~0ull;
    }
  }
  return L.bytes();
}

// at<T>: the address of a piece is base + off, typed -> the distance in bytes from base
uint64_t sfl_carve_at(uint64_t off) {
  static uint8_t base[64];
  return (uint64_t)((uint8_t*)sf::stage::Carve::at<uint32_t>(base, (size_t)off) - base);
}

// the stream driver's chunk scratch as stream_batch_run carves it: cand u64[nc] | recs StreamChunk[nc] | list u32[nc]
// -> out[0..2] the offsets, out[3] the total (what sfh_last_stream_stats reports), out[4] sizeof(StreamChunk)
void sfl_stream_scratch(uint64_t nc, uint64_t* out) {
  sf::stage::Carve C;
  out[0] = C.add<uint64_t>((size_t)nc);
  out[1] = C.add<sf::StreamChunk>((size_t)nc);
  out[2] = C.add<uint32_t>((size_t)nc);
  out[3] = C.bytes();
  out[4] = sizeof(sf::StreamChunk);
}
}
