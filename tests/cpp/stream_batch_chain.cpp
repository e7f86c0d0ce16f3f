// Host shim for tests/test_stream_batch_chain.py: the chain round of sf_stream_chain.h, which the stream decoder runs over each
// item's slice of the call's records, and the same round over one stream's records alone (r0 = 0), on the same record layout.
// TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_stream_chain.h"

#include <cstring>

extern "C" {

// one round over rec[r0, r0 + m): appends to redo (indices into rec) -> the number appended; *chain: confirmed records
uint32_t sfb_chain_round_slice(sf::StreamChunk* rec, uint32_t r0, uint32_t m, uint32_t* redo, uint32_t* chain) {
  std::vector<uint32_t> r;
  sf::stream_chain_round(rec, r0, m, r, chain);
  if (!r.empty()) std::memcpy(redo, r.data(), 4 * r.size());
  return static_cast<uint32_t>(r.size());
}

// one round over the m records of one stream (a slice with r0 = 0) -> the number to decode again
uint32_t sfb_chain_round_vector(sf::StreamChunk* rec, uint32_t m, uint32_t* redo, uint32_t* chain) {
  std::vector<uint32_t> r;
  sf::stream_chain_round(rec, 0, m, r, chain);
  if (!r.empty()) std::memcpy(redo, r.data(), 4 * r.size());
  return static_cast<uint32_t>(r.size());
}
}
