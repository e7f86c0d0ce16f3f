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

// A file of gzip members (SFH_GZIP_MEMBERS): what a chunk knows about the members that end inside it stands beside its record,
// in a row of its own.  Behind the count pass: n members closed, the last of them at byte `at` of the chunk's output.  For the
// write pass the host turns that into: the member open at the chunk's start began at byte `at` of the item's output, and the
// chunk's n member rows start at row `first` of the call's.
struct StreamSide {
  uint64_t at;
  uint32_t n, first;
};
// One row per member, in file order (sfh_debug_read's SFH_DBG_STREAM_MEMBERS record): offsets from the item's first byte.
struct StreamMember {
  uint64_t src_end;  // just past its trailer
  uint64_t out_end;  // just past its output
  uint32_t crc32, isize;  // its trailer's values
  uint32_t item;     // the write pass: its item's row; the host: its item in the call
  uint32_t status;   // 0, or 1: the trailer does not match the output
};
static_assert(sizeof(StreamSide) == 16 && sizeof(StreamMember) == 32, "member rows");

// After the chain rounds, over an item's confirmed records rec[r0, r0 + chain) and their side rows: the rows as the write pass
// reads them (a record that a round settled as empty closes nothing, whatever its stale row says).  first: the item's first
// member row; returns the row behind its last.
inline uint64_t stream_member_scan(const StreamChunk* rec, StreamSide* side, uint32_t r0, uint32_t chain, uint64_t first) {
  uint64_t open_at = 0;  // where the open member began in the item's output
  for (uint32_t i = r0; i < r0 + chain; ++i) {
    const uint32_t n = rec[i].start >= rec[i].limit ? 0u : side[i].n;
    const uint64_t closed_at = rec[i].base + side[i].at;
    side[i] = StreamSide{open_at, n, (uint32_t)first};
    if (n) open_at = closed_at;
    first += n;
  }
  return first;
}

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
