// sf_stream_chain.h -- the chunk record of the stream decoder (sf_stream.hip) and step C, the chain round, in plain C++ so that
// the host tests run the code the library runs (tests/cpp/stream_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

namespace sf {

// Bit positions are body bits (the stream without its wrapper); limit: where the chunk's decode stops (at its first block end
// at or beyond it); base: O_i, its output offset.
struct StreamChunk {
  uint64_t start, limit, end, out, base;
  uint32_t status, final_;
};
static_assert(sizeof(StreamChunk) == 48, "stream chunk record");

// C on the host: one round over the chunk records rec[r0, r0 + m) of one stream (rec[i].start / .limit are the chunks as
// decoded; an empty chunk is settled here).  Appends the chunks to decode again to redo (indices into rec); *chain: the
// confirmed chunks so far (the last one ends the stream or failed) when none was appended.  A call keeps every item's records
// in one array and runs this over each item's slice (one stream: r0 = 0).
inline void stream_chain_round(StreamChunk* rec, uint32_t r0, uint32_t m, std::vector<uint32_t>& redo, uint32_t* chain) {
  uint32_t confirmed = 1;
  bool broken = false;
  for (uint32_t i = 0; i + 1 < m; ++i) {
    StreamChunk& a = rec[r0 + i];
    if (a.status != 0 || a.final_) {
      if (!broken) break;  // the chain ends here
      continue;
    }
    if (a.end != rec[r0 + i + 1].start) {
      StreamChunk& b = rec[r0 + i + 1];
      b.start = a.end;
      a.limit = a.end;  // (a stopped at its first block end at or beyond it: the same decode)
      if (b.start >= b.limit) {  // nothing of b's range is left: an empty chunk, settled here
        b.end = b.start;
        b.out = 0;
        b.status = 0;
        b.final_ = 0;
      } else {
        redo.push_back(r0 + i + 1);
        broken = true;
        ++i;  // b's record is stale until it is decoded again
        continue;
      }
    }
    if (!broken) ++confirmed;
  }
  *chain = confirmed;
}

// The same over all of rec (one stream).  Returns the chunks to decode again.  The library runs the slice form only; this one
// is for host-side callers that hold one stream's records in a vector.
inline std::vector<uint32_t> stream_chain_round(std::vector<StreamChunk>& rec, uint32_t* chain) {
  std::vector<uint32_t> redo;
  stream_chain_round(rec.data(), 0, (uint32_t)rec.size(), redo, chain);
  return redo;
}

}  // namespace sf
