// Host shim for tests/test_stream_batch_chain.py: the per-item chain round of sf_stream_chain.h (the overload the batched
// stream decoder runs over each item's slice of the call's records) and the one-stream round, on the same record layout.
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

// one round over the m records of one stream (the std::vector overload) -> the number to decode again
uint32_t sfb_chain_round_vector(sf::StreamChunk* rec, uint32_t m, uint32_t* redo, uint32_t* chain) {
  std::vector<sf::StreamChunk> v(rec, rec + m);
  const std::vector<uint32_t> r = sf::stream_chain_round(v, chain);
  if (m) std::memcpy(rec, v.data(), sizeof(sf::StreamChunk) * m);
  if (!r.empty()) std::memcpy(redo, r.data(), 4 * r.size());
  return static_cast<uint32_t>(r.size());
}
}
