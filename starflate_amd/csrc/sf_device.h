// sf_device.h -- device-side data layout shared by the kernels and the C-ABI host.
//
// Pipeline (one HIP stream, four launches per call):
//   K1 k_lz77   one 1024-thread workgroup per STRIP (block_bytes of input, a whole number of 32 KiB
//               chunks, coded independently of what precedes it): a 32 KiB window + the 8 KiB round in
//               flight + the hash table + per-position (len,dist) of the round in LDS; step-synchronous
//               hash insertion (two history levels per bucket), candidate compare, wave-local
//               register-resident greedy/lazy parse; 16-bit token items + histogram out, one DEFLATE
//               block per chunk.  Other match phases behind the same stage / parse / emit: exact hash chains
//               (SFH_EFFORT_BEST ..: heads + links in LDS, one workgroup per CU) and the step tables filled in
//               position order (SFH_EFFORT_RECENT / _RECENT_ALL: buckets {lo, hi}, the exact predecessor as a
//               candidate); both insert 64 positions per returning LDS atomic and rest on the lane order
//               sf_guard.hip checks at run time
//   K2 k_plan   one wave per chunk: raw length counts folded into symbols, length-limited Huffman lengths (ll, d, cl),
//               canonical codes, dynamic header bits, block type, exact byte size
//   K3 k_scan   exclusive scan of chunk byte sizes -> output offsets, total
//   K4 k_emit   one workgroup per chunk: bit-pack tokens into LDS, flush to the
//               chunk's final byte offset (or copy raw bytes for a stored block)
// With a zlib / gzip container two more launches (sf_checksum.hip):
//   K5 k_checksum  one workgroup per chunk: Adler-32 / CRC-32 partial of the chunk's input bytes
//   K6 k_wrap      one workgroup: fold the partials, write wrapper header + trailer
// A call on more than kBatchChunks chunks runs K1..K4 batch after batch (bounded scratch); the host-buffer entry
// point pipelines smaller batches with their copies.  A batched call (sfh_compress_batch*: many items, each its own
// stream) runs the same kernels over descriptor tables (BatchStrip / BatchChunk / BatchItem below).
// The decoder (sf_inflate.hip, sf_inflate_core.h) runs the other way, over descriptor rows (InflateSeg / InflateStrip / InflateItem
// below): k_inflate_tokens[_sub / _spec] (Huffman codes -> tokens, all segments at once), k_inflate_bytes (tokens -> bytes,
// strip by strip), k_inflate_fold (every item's status).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "sf_stream_chain.h"

namespace sf {

constexpr uint32_t kChunk = 32768;      // bytes per DEFLATE block (byte-aligned in the stream)
constexpr uint32_t kWindow = 32768;     // a match reaches back at most this far, and never before its strip
constexpr uint32_t kWideRow = 65536;    // the decoder's wide rows: a foreign BGZF member's output (bgzip: 65280), and its tokens
constexpr uint32_t kStep = 1024;        // positions per hash-insertion step (= K1 threads)
constexpr uint32_t kHashBits = 13;      // buckets of two 16-bit history levels each (32 KiB of LDS)
constexpr uint32_t kMaxStrip = 1u << 24;  // largest block_bytes
constexpr uint32_t kRegion = 512;       // parse region: matches never cross it (one wave of k_lz77 parses one)
constexpr uint32_t kSubBytes = 1024;    // sub-index granularity: every kSubBytes-th position starts a token
constexpr uint32_t kCap = 16;           // match-time compare width; longer matches are extended by the parse
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kFar4 = 4096;        // a match of exactly 4 bytes beyond this distance is not used
constexpr uint32_t kSkipSlack = 128;    // stored fast path: first 8 KiB with >= 8192-128 tokens => no further search
constexpr uint32_t kSkipProbe = 2048;   // ... and behind such a chunk in its strip only this many positions of the 8 KiB are searched
constexpr uint32_t kItemsSkipped = 0x80000000u;  // nitems[chunk]: the items were not written -- they are the chunk's own bytes
                                                 // (stored fast path: every position a literal); k_emit takes them from the input
constexpr uint32_t kSubRegions = kChunk / kSubBytes;  // 32 sub-index entries per chunk
constexpr uint32_t kTokMatch = 0x80000000u;  // decoder token (k_inflate_*): bit31 match, 16..23 len-3, 0..14 dist-1
constexpr uint32_t kTokRegion = 0x40000000u; // decoder token: first token of a parse region, region index in 24..28
// k_lz77 -> k_emit: 16-bit ITEMS, at most kChunk per chunk.  A literal is one item (kItemTok | byte); a match is two:
// head = kItemTok | kItemHead | len-3, then dist-1 (15 bits, bit 15 clear).  Every item says what it is by itself (round 6;
// before, a distance was "the item behind a head" and k_emit looked at every item's neighbour), and kItemHead sits right
// above the byte: a token's low nine bits ARE its place in k_emit's table of literal and length codes.  The first item of a
// parse region's first token also carries kItemRegion and the region's index in bits 9..13 (kItemRegionShift): the format's
// own record of the region starts (debug_tokens, the tests).  k_emit does not look for the flag: k_lz77 hands it the item
// index of every region's first token beside the region's token count (Workspace::rtok, a region_word).
constexpr uint32_t kItemTok = 0x8000u;     // a token's first item: a literal or a match head (clear: a distance)
constexpr uint32_t kItemRegion = 0x4000u;
constexpr uint32_t kItemRegionShift = 9;
constexpr uint32_t kItemHead = 0x0100u;    // with kItemTok: a match head (len-3 in bits 0..7)
// Workspace::rtok's word for one region: the tokens before it (low half) and the items before it (high half)
static_assert(kChunk <= 0x8000u, "a chunk's token and item counts fit 16 bits each");
constexpr uint32_t region_word(uint32_t tokens_before, uint32_t items_before) { return tokens_before | (items_before << 16); }

constexpr uint32_t kChecksumAdler32 = 1;  // = SFH_ZLIB
constexpr uint32_t kChecksumCrc32 = 2;    // = SFH_GZIP
constexpr uint32_t kCrcPoly = 0xEDB88320u;  // RFC 1952 section 8, reflected

constexpr uint32_t kHistStride = 576;   // ll[0..285] at 0, d[0..29] at 288, raw len-3 counts [0..255] at 320
constexpr uint32_t kHistD = 288;
constexpr uint32_t kHistLen = 320;      // k_lz77 counts match lengths raw; k_plan folds them into ll[257..285]
constexpr uint32_t kHeaderWords = 152;  // 608 bytes >= 4495-bit worst-case dynamic header + 3

// Wave-wide scans on the DPP network (no LDS round trips), for the encoder's and the decoder's kernels alike.  Identity 0;
// a lane whose source does not exist keeps the identity (`old` operand, bound_ctrl off).  row_shr:n = 0x110+n,
// row_bcast:15 = 0x142 (rows 1 and 3), row_bcast:31 = 0x143 (rows 2 and 3), wave_shr:1 = 0x138.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_from(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add_from(uint32_t v) {
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
  v = dpp_add_from<0x111, 0xF>(v);
  v = dpp_add_from<0x112, 0xF>(v);
  v = dpp_add_from<0x114, 0xF>(v);
  v = dpp_add_from<0x118, 0xF>(v);
  v = dpp_add_from<0x142, 0xA>(v);
  v = dpp_add_from<0x143, 0xC>(v);
  return v;
}
__device__ __forceinline__ uint32_t wave_excl_max(uint32_t v) {
  v = max(v, dpp_from<0x111, 0xF>(v));
  v = max(v, dpp_from<0x112, 0xF>(v));
  v = max(v, dpp_from<0x114, 0xF>(v));
  v = max(v, dpp_from<0x118, 0xF>(v));
  v = max(v, dpp_from<0x142, 0xA>(v));
  v = max(v, dpp_from<0x143, 0xC>(v));
  return dpp_from<0x138, 0xF>(v);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_add(v), 63);
}

// A pointer read from a row is a generic one to the compiler, and a load through it a FLAT load, which counts on lgkmcnt as
// well as on vmcnt: k_inflate_tokens' waits for its LDS reads then also wait for the window loads in flight (token stage of a
// 1 GiB stream, sub-indexed: 3.24 ms against 2.97 with the stream pointer a kernel argument).  Rows point to device
// memory; said here, where a kernel takes a pointer out of its row, the accesses are global ones.
template <class T>
__device__ __forceinline__ T* row_ptr(T* p) {
  return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

// per-chunk plan record written by K2, read by K3/K4
struct ChunkPlan {
  uint32_t btype;        // 0 stored, 1 fixed, 2 dynamic
  uint32_t out_bytes;    // exact bytes of this chunk in the stream
  uint32_t header_bits;  // bits in `header` (block header 3 bits + dynamic header)
  uint32_t body_bits;    // token bits + EOB
};
struct ChunkCodes {
  uint32_t lcode[288];   // bit-reversed code | nbits << 16
  uint32_t dcode[32];
  uint32_t header[kHeaderWords];  // LSB-first bitstream: BFINAL,BTYPE, then RFC 1951 3.2.7 header
  uint8_t lens[320];     // ll lens [0..287], d lens [288..319] (debug / parity)
};

// k_plan in three launches (round 6): what the sorting pass hands the merge pass and the merge pass the finishing one, per chunk
struct PlanTree {
  uint32_t done;           // 1: the sorting pass settled the chunk (stored without a code)
  uint32_t m_ll, m_d;      // used literal/length and distance symbols
  uint32_t pad;
  uint32_t key_ll[288];    // (freq << 9 | symbol) ascending, [0 .. m_ll)
  uint32_t key_d[32];
  uint16_t wt_ll[288];     // the same symbols' weights (what the merge reads)
  uint16_t wt_d[32];
  uint16_t parent_ll[576]; // the merge's result: node -> parent, root = node 2m - 2
  uint16_t parent_d[64];
};
static_assert(sizeof(PlanTree) % 16 == 0, "PlanTree rows");

// per-segment record of the decoder (sf_inflate.hip): written by k_inflate_tokens*, read by k_inflate_bytes and k_inflate_fold
constexpr uint32_t kSegRaw = 1u, kSegSerial = 2u;
struct SegInfo {
  uint32_t status;   // DecompressStatus of the reference (src/decompress.hpp:13-23), 0 = Success
  uint32_t ntok;
  uint32_t raw;      // bit 0 (kSegRaw): one stored block holding the whole segment, bytes at raw_off of the stream;
                     // bit 1 (kSegSerial): decoded by the lane-serial kernel (diagnostic, SFH_DBG_SEGINFO)
  uint32_t out_n;    // bytes this segment produces
  uint64_t raw_off;
};

// Arrays marked (batch) hold one batch of at most kBatchChunks chunks: a call on a larger input runs the four kernels
// batch after batch on the same stream, so the scratch of a call is bounded (2.2 bytes per input byte of one batch).
constexpr uint32_t kBatchChunks = 32768;  // 1 GiB of input

struct Workspace {
  uint16_t* items;    // (batch) [nchunks][kChunk] token items (K1 -> K4)
  uint32_t* nitems;   // [nchunks]
  uint32_t* tokens;   // [nseg][kChunk] decoder only (k_inflate_tokens* -> k_inflate_bytes)
  uint32_t* ntok;     // [nchunks] tokens (a match counts once)
  uint32_t* hist;     // [nchunks][kHistStride]
  ChunkPlan* plan;    // [nchunks]
  ChunkCodes* codes;  // [nchunks]
  PlanTree* ptree;    // (batch) [nchunks] k_plan's three launches hand their chunk's tree along here
  uint64_t* offsets;  // [nchunks + 1]: first stream byte of every chunk, then the end of the last one (= the index)
  uint64_t* stamps;   // [nchunks][8], diagnostic build only (SFH_K1_STAMPS=1), else null
  uint32_t* sums;     // [nchunks] checksum partials (container modes / sfh_checksum_device)
  SegInfo* seginfo;   // [nchunks] decoder only
  uint32_t* rtok;     // (batch) [nchunks][32] region_word: tokens | items << 16 before each 1024-byte parse region (K1 -> K4)
  uint32_t* subidx;   // [nchunks][32][2] sub-index: {bit offset of the region's first code, tokens before it}
};

struct Options {
  uint32_t strategy;
  uint32_t final_stream; // 1: the call's last chunk ends with BFINAL; 2 (BGZF): every chunk does
  uint32_t lazy;
  uint32_t fast_skip;     // 0: off; 1: stored fast path; 2: ... and a chunk may be stored by its probe (strategy 0 only: launch_lz77)
  uint32_t strip_bytes;  // multiple of kChunk
  uint32_t depth2;       // 1: both history levels of a hash bucket are tried, 0: the newer one only
  uint32_t near;         // 1: the step-local candidate is tried as well (always with depth2)
  uint32_t stride2;      // 1: only even positions are searched, odd ones take over their successor's match (0: thorough)
  uint32_t long_table;   // 1: two tables of 4096 buckets, keyed by four and by seven bytes (with stride2 = 0: SFH_EFFORT_MAX)
  uint32_t chain_depth;  // > 0: exact hash chains of this depth instead of the step tables (SFH_EFFORT_BEST 8, _ULTRA 16, _EXTREME 32)
  uint32_t recent;       // 1: exact recency (SFH_EFFORT_RECENT): buckets {latest, the one before the latest inserting step} + the exact predecessor
};

// Batched compression (sfh_compress_batch*): many independent items, each its own stream, in one launch batch.  The
// host's descriptor tables stand in for the single call's implicit geometry (strip = blockIdx.x * strip_bytes, chunk =
// blockIdx.x * kChunk of one input, BFINAL on the last chunk of the launch).
struct BatchStrip {   // per strip of the launch batch (k_lz77)
  const uint8_t* src; // the strip's first byte (16-byte aligned)
  uint32_t n;         // its bytes
  uint32_t chunk0;    // its first chunk in the launch batch
};
struct BatchChunk {   // per chunk (k_plan, k_emit; k_checksum over the whole call)
  const uint8_t* src; // the chunk's first byte
  uint32_t n_raw;     // its bytes (0: an empty item's one chunk)
  uint32_t item;      // index into the launch batch's item table << 1 | 1 on the last chunk of its item
};
struct BatchItem {    // per item (or piece of an item) in the launch batch (k_scan, k_emit)
  uint8_t* dst;       // the item's stream
  uint64_t shift;     // written by k_scan: stream offset of a chunk = its offset in the batch's global scan + shift
  uint32_t out;       // the item's index in the call (d_out_n[out])
  uint32_t chunk0;    // its first chunk in the launch batch
  uint32_t nchunks;   // its chunks in the launch batch
  uint32_t carry;     // 1: a piece after the item's first: its stream goes on from d_out_n[out]
};
struct WrapItem {     // per item of the call (the batched k_checksum / k_wrap)
  uint8_t* dst;
  uint64_t n;         // the item's bytes
  uint32_t out;
  uint32_t sum0;      // its first chunk's checksum partial
  uint32_t nchunks;
  uint32_t pad;
};
struct BatchIndexRow { // per chunk of the call (k_batch_index: the batch's index, sfh_copy_batch_index)
  uint32_t piece;     // its row in the call's item table (the piece of its item in one launch batch)
  uint32_t item;      // its item's index in the call
};
static_assert(sizeof(BatchStrip) == 16 && sizeof(BatchChunk) == 16 && sizeof(BatchItem) == 32 && sizeof(WrapItem) == 32,
              "descriptor rows (the host packs them into one upload)");
// The indexed decoder (sfh_decompress*, sfh_decompress_batch*, _range*, _any*): its kernels read a segment's stream, index
// entries, output and history from these rows (a single stream is a call of one item; the cut into launch batches:
// sf_inflate_plan.h).
struct InflateSeg {      // per segment of a launch batch (k_inflate_tokens*, k_inflate_bytes)
  const uint8_t* src;    // its item's stream (index entries are offsets into it)
  const uint64_t* ix;    // its two index entries: [ix[0], ix[1]) are its stream bytes
  const uint32_t* sub;   // its SFH_SUBINDEX_WORDS sub-index words (k_inflate_tokens_sub only)
  uint8_t* dst;          // its first output byte (16-byte aligned)
  uint64_t src_n;        // stream bytes the decoder may read (a wrapped item: its trailer excluded)
  uint32_t out_n;        // output bytes
  uint32_t hist;         // bytes of its strip before it (how far back a match may reach beyond it) | kSegWrapped
};
constexpr uint32_t kSegWrapped = 0x80000000u;  // InflateSeg.hist: a zlib / gzip item's segment (a body that ends short is Error)
constexpr uint32_t kSegExact = 0x40000000u;    // InflateSeg.hist, recovered index only (launch_inflate_tokens_exact): not the
                                               // stream's last segment, so its blocks must end on its last byte
struct InflateStrip {    // per strip of a launch batch (k_inflate_bytes: one workgroup each)
  uint32_t seg0, nseg;   // its first segment in the launch batch, its segments
};
struct InflateItem {     // per item of the call (k_inflate_head, k_inflate_fold)
  const uint8_t* src;
  uint64_t src_n;
  uint64_t dst_n;
  uint64_t* implied;     // index-free call: where k_inflate_head writes the item's two index entries (null: an index is given)
  const uint64_t* ix0;   // with an index: the item's first entry (checked against the wrapper header's end)
  uint32_t seg0, nseg;   // its first segment in the call's segment records (and checksum partials), its segments
  uint32_t wst;          // written by k_inflate_head: the wrapper's status (0: in order)
  uint32_t want;         //   the checksum the trailer carries
  uint32_t isize;        //   gzip: ISIZE
  uint32_t pad;
};
static_assert(sizeof(InflateSeg) == 48 && sizeof(InflateStrip) == 8 && sizeof(InflateItem) == 64, "decoder descriptor rows");
// Random access (sfh_decompress_range*; sf_range_plan.h): the rows of a launch batch are the segments of the ranges' decode
// spans, and beside every InflateSeg stands its write window -- the part of the segment that belongs to the range.
struct InflateClip {     // per segment of a launch batch (k_inflate_bytes_clip)
  uint8_t* dst;          // where its byte `lo` goes (any alignment)
  uint32_t lo, hi;       // [lo, hi) of its out_n bytes are written; lo == hi: it is resolved in LDS only
};
struct InflateSpan {     // per range of the call (k_inflate_fold_spans)
  uint32_t row0, nrows;  // its rows in the call's segment records
};
static_assert(sizeof(InflateClip) == 16 && sizeof(InflateSpan) == 8, "range descriptor rows");
// The reference's DecompressStatus values the wrapper checks produce (src/decompress.hpp:13-23).
namespace gz {
constexpr uint32_t kStOk = 0, kStError = 1, kStDstTooSmall = 4, kStSrcTooSmall = 5;
}
// the gzip wrapper of the n bytes at p (any alignment) whose body decodes into dst_n bytes: container.hpp's checks in its
// order.  st, hdr, end (= n), want and isize come in cleared
__device__ __forceinline__ void gzip_head(const uint8_t* __restrict__ p, uint64_t n, uint64_t dst_n, uint32_t& st, uint64_t& hdr,
                                          uint64_t& end, uint32_t& want, uint32_t& isize) {
  if (n < 18) {
    st = gz::kStSrcTooSmall;
  } else if (p[0] != 0x1F || p[1] != 0x8B || p[2] != 8 || (p[3] & 0xE0u) != 0) {
    st = gz::kStError;
  } else {
    const uint32_t flg = p[3];
    end = n - 8;
    uint64_t at = 10;
    if (flg & 0x04u) {  // FEXTRA
      if (at + 2 > end) st = gz::kStSrcTooSmall;
      else at += 2 + (p[at] | (uint32_t)p[at + 1] << 8);
    }
    for (uint32_t bit = 0x08u; st == gz::kStOk && bit <= 0x10u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
      if (!(flg & bit)) continue;
      while (at < end && p[at] != 0) ++at;
      ++at;
    }
    if (flg & 0x02u) at += 2;  // FHCRC
    if (st == gz::kStOk && at > end) st = gz::kStSrcTooSmall;
    hdr = at;
    want = p[n - 8] | (uint32_t)p[n - 7] << 8 | (uint32_t)p[n - 6] << 16 | (uint32_t)p[n - 5] << 24;
    isize = p[n - 4] | (uint32_t)p[n - 3] << 8 | (uint32_t)p[n - 2] << 16 | (uint32_t)p[n - 1] << 24;
    if (st == gz::kStOk && isize > dst_n) st = gz::kStDstTooSmall;
  }
}

struct BatchTables {  // the device tables of one launch batch (null: the single call's implicit geometry)
  const BatchStrip* strips;
  uint32_t nstrips;
  const BatchChunk* chunks;
  BatchItem* items;
  uint32_t nitems;
};

hipError_t launch_lz77(const uint8_t* src, uint64_t n, uint32_t nchunks, const Workspace& ws,
                       const Options& opt, hipStream_t s, const BatchTables* bt = nullptr);
hipError_t launch_plan(uint64_t n, uint32_t nchunks, const Workspace& ws, const Options& opt,
                       hipStream_t s, const BatchTables* bt = nullptr);
// offsets start at `base` (bytes of wrapper header in front of the stream), or with `carry` at the current *d_total
// (the end of the previous batch); *d_total = the end of this batch.  With tables: every item's offsets start at `base`
// (or, carried, at d_total[item.out]) and d_total[item.out] = the end of the item's stream so far
// lead, extra (BGZF, without tables): every chunk a member of `extra` bytes around its block, the offsets `lead` bytes behind the
// members' first bytes (see k_scan)
hipError_t launch_scan(uint32_t nchunks, const Workspace& ws, uint64_t base, bool carry, uint64_t* d_total, hipStream_t s,
                       const BatchTables* bt = nullptr, uint32_t lead = 0, uint32_t extra = 0);
hipError_t launch_emit(const uint8_t* src, uint64_t n, uint32_t nchunks, const Workspace& ws, const Options& opt,
                       uint8_t* dst, hipStream_t s, const BatchTables* bt = nullptr);
// after every launch batch of a batched call: the items' index entries (item-relative offsets, item after item) into `index`
hipError_t launch_batch_index(const BatchChunk* chunks, const BatchIndexRow* rows, const BatchItem* pieces, const uint64_t* offsets,
                              const uint64_t* total, uint32_t nchunks, uint64_t* index, hipStream_t s);
hipError_t init_kernels();

// sf_checksum.hip
// bytes in front of the raw stream; nseg != 0 (gzip only): the dictzip header with its table of nseg chunk sizes
uint32_t wrapper_header_bytes(uint32_t kind, uint32_t nseg = 0);
hipError_t launch_checksum(const uint8_t* src, uint64_t n, uint32_t nchunks, uint32_t kind, uint32_t* sums,
                           hipStream_t s);
// dst != null: header at dst[0..), trailer at dst[*d_total..), *d_total += trailer bytes; d_value (nullable) = checksum
// dz_offsets (gzip, dst 4-byte aligned; null: the plain header): the call's index -- the header is dictzip's (sf_dz_plan.h)
hipError_t launch_wrap(const uint32_t* sums, uint32_t nchunks, uint64_t n, uint32_t kind, uint8_t* dst,
                       uint64_t* d_total, uint32_t* d_value, hipStream_t s, const uint64_t* dz_offsets = nullptr);
// the dictzip table of a gzip stream read into index[0 .. nseg] (k_dz_index); *out: sfh_dz_info's fields, then the return code
struct DzInfo {
  uint64_t total_n;
  uint32_t nseg, header_bytes, status;
  int32_t rc;
};
hipError_t launch_dz_index(const uint8_t* src, uint64_t src_n, uint64_t* index, uint64_t index_cap, DzInfo* out, hipStream_t s);
// BGZF (sf_bgzf_plan.h).  The writer: behind a launch batch's k_emit and k_checksum (k_scan ran with lead 18, extra 26), one lane
// per member stores its header and trailer; eof: the EOF member at *d_total, which grows by it (2: at 0, the whole file)
hipError_t launch_bgzf_wrap(const uint32_t* sums, const uint64_t* offsets, uint32_t nmembers, uint64_t n, uint8_t* dst,
                            uint64_t* d_total, uint32_t eof, hipStream_t s);
// The reader (sf_bgzf.hip): *out of the walk -- sfh_bgzf_info's fields, the return code, and whether a member's output starts
// off a 16-byte boundary
struct BgzfInfo {
  uint64_t total_n;
  uint32_t members, max_isize, has_eof, status;
  int32_t rc;
  uint32_t unaligned, pad;
};
uint32_t bgzf_scan_blocks(uint64_t src_n);  // workgroups (counts) of the node scan
hipError_t launch_bgzf_count(const uint8_t* src, uint64_t src_n, uint32_t* cnt, hipStream_t s);
size_t bgzf_walk_bytes(uint32_t nn);        // scratch of the walk over nn nodes
// node_off: the exclusive scan of the counts, nn their total.  member_off, out_off: cap entries each, written when the file
// parses and members + 1 <= cap
hipError_t launch_bgzf_walk(const uint8_t* src, uint64_t src_n, const uint32_t* node_off, uint32_t nn, uint8_t* scratch,
                            uint64_t* member_off, uint64_t* out_off, uint64_t cap, BgzfInfo* out, hipStream_t s);
// the decoder's rows for members of one segment each (see k_bgzf_rows); the first failing member: res[0] its status, res[1] it
hipError_t launch_bgzf_rows(const uint8_t* src, const uint64_t* member_off, const uint64_t* out_off, uint32_t nmembers,
                            uint32_t per_batch, uint8_t* dst, InflateSeg* segs, InflateItem* items, InflateClip* clips,
                            InflateStrip* strips, BatchChunk* sums, uint64_t* implied, hipStream_t s);
// ... for members of up to kWideRow bytes: TWO checksum rows per member (sums[2 i], sums[2 i + 1]: its first 32 KiB, the rest)
hipError_t launch_bgzf_rows_wide(const uint8_t* src, const uint64_t* member_off, const uint64_t* out_off, uint32_t nmembers,
                                 uint32_t per_batch, uint8_t* dst, InflateSeg* segs, InflateItem* items, InflateClip* clips,
                                 InflateStrip* strips, BatchChunk* sums, uint64_t* implied, hipStream_t s);
hipError_t launch_bgzf_first(const uint32_t* status, uint32_t m, uint32_t* res, hipStream_t s);
// BGZF random access (sfh_decompress_bgzf_ranges*; sf_bgzf_range_plan.h).  One row per range of the call, built by the host:
struct BgzfRange {
  uint64_t offset, length;  // of the file's output
  uint8_t* dst;             // any alignment
  const uint8_t* src;       // the FILE's byte 0 as this range's rows see it (the host-buffer call: a base in front of the
  uint64_t src_lo, src_n;   // span's uploaded piece), and the bytes [src_lo, src_n) of the file that are readable from it
};
static_assert(sizeof(BgzfRange) == 48, "range rows (the host packs them into one upload)");
// plan[0 .. n): every range's first member, plan[n .. 2n): its rows (0 and first = 0xFFFFFFFF: a range the index does not
// hold); *total (64-bit, zeroed by the launch) = the rows of the call
hipError_t launch_bgzf_range_spans(const BgzfRange* ranges, uint32_t n, const uint64_t* out_off, uint32_t members, uint32_t* plan,
                                   unsigned long long* total, hipStream_t s);
// row0: the exclusive scan of the rows.  Per row its InflateSeg, write window, strip of one (numbered within its launch batch
// of per_batch rows), implied entries and wrapper status; per range its InflateSpan.  row_bytes: kChunk or kWideRow
hipError_t launch_bgzf_range_rows(const BgzfRange* ranges, uint32_t n, const uint64_t* member_off, const uint64_t* out_off,
                                  const uint32_t* plan, const uint32_t* row0, uint32_t nrows, uint32_t per_batch, uint32_t row_bytes,
                                  InflateSeg* segs, InflateClip* clips, InflateStrip* strips, uint64_t* implied, uint32_t* wst,
                                  InflateSpan* spans, hipStream_t s);
// every range's status: the first failing row of its span, a row's wrapper status before its body's; 1 for a range the
// planner marked failed
hipError_t launch_bgzf_fold_spans(const InflateSpan* spans, uint32_t n, const uint32_t* plan, const SegInfo* info, const uint32_t* wst,
                                  uint32_t* status, hipStream_t s);
// the batched fold alone (sfh_compress_zip*): crc[items[i].out] = the CRC-32 of item i from its chunks' partials
hipError_t launch_crc_items(const uint32_t* sums, const WrapItem* items, uint32_t nitems, uint32_t* crc, hipStream_t s);
hipError_t launch_checksum_batch_any(const BatchChunk* chunks, uint32_t nchunks, uint32_t* sums, hipStream_t s);  // CRC-32, any alignment
// batched: sums[c] for the call's chunk table; one k_wrap workgroup per item (header at dst, trailer at d_total[out])
hipError_t launch_checksum_batch(const BatchChunk* chunks, uint32_t nchunks, uint32_t kind, uint32_t* sums, hipStream_t s);
hipError_t launch_wrap_batch(const uint32_t* sums, const WrapItem* items, uint32_t nitems, uint32_t kind,
                             uint64_t* d_total, hipStream_t s);
// sf_inflate.hip
hipError_t init_inflate_kernels();
// one launch batch: its segment rows (info and tokens: the batch's own), then its strips (a segment's matches may reach its
// strip's earlier segments).  sub: the rows carry sub-index words; else speculate, or the lane-serial kernel alone
hipError_t launch_inflate_tokens(const InflateSeg* rows, uint32_t nseg, uint32_t* tokens, SegInfo* info, bool sub, bool speculate,
                                 hipStream_t s);
hipError_t launch_inflate_bytes(const InflateSeg* rows, const InflateStrip* strips, uint32_t nstrips, const uint32_t* tokens,
                                SegInfo* info, hipStream_t s);
// the same two stages on wide rows: segments of up to kWideRow bytes, tokens [nseg][kWideRow], index only; clips: null, or
// every row's write window
hipError_t launch_inflate_tokens_wide(const InflateSeg* rows, uint32_t nseg, uint32_t* tokens, SegInfo* info, bool speculate,
                                      hipStream_t s);
hipError_t launch_inflate_bytes_wide(const InflateSeg* rows, const InflateClip* clips, const InflateStrip* strips, uint32_t nstrips,
                                     const uint32_t* tokens, SegInfo* info, hipStream_t s);
// ---- sf_unindexed.hip: the segment index recovered from the stream ----
uint32_t any_scan_waves(uint64_t src_n);  // waves (per-wave counts) of k_any_scan over a buffer of src_n bytes
size_t any_scan_tmp_words(uint32_t n);    // words of `tmp` launch_scan_u32 needs for n elements
// exclusive scan of n uint32 (in-place allowed); *total: their sum (device)
hipError_t launch_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tmp, uint32_t* total, hipStream_t s);
// The bodies of a call (one stream is a call of one item): the scan runs one wave per 8 KiB of one item (waves: the wave ->
// {item, piece} map, built by the host), the node list is the items' lists one after the other, each with its own end
// sentinel, and the walk stays inside a node's item (range[item], written by launch_any_ranges).  heads: every item's body
// [b0, e) (k_inflate_head's implied entries); index: flat, item i's nseg + 1 entries from items[i].ix0.
struct AnyItem {
  const uint8_t* src;
  uint64_t src_n;
  uint64_t ix0;            // its first entry in the flat index
  uint32_t nseg;
  uint32_t wave0, nwaves;  // its waves in the call (none: an item of one segment, which needs no walk)
  uint32_t pad;
};
struct AnyWave {
  uint32_t item, piece;    // the wave scans bytes [piece * 8192, +8192) of the item's stream
};
struct AnyRange {
  uint32_t n0, n1, m0, m1; // the item's nodes [n0, n1) and its sentinel n1; its M nodes [m0, m1) of the M list
};
static_assert(sizeof(AnyItem) == 40 && sizeof(AnyWave) == 8 && sizeof(AnyRange) == 16, "recovery descriptor rows");
// count: nodes and M nodes per wave; nodes: write them (offsets = exclusive scans of the counts)
hipError_t launch_any_count(const AnyItem* items, const AnyWave* waves, const uint64_t* heads, uint32_t nwaves, uint32_t* cnt_nodes,
                            uint32_t* cnt_m, hipStream_t s);
// after the scans of the counts (tot[0], tot[1]: their totals): range[], and *largest = the largest item's nodes (zeroed before)
hipError_t launch_any_ranges(const AnyItem* items, uint32_t nitems, const uint32_t* node_off, const uint32_t* m_off, uint32_t nwaves,
                             const uint32_t* tot, AnyRange* range, uint32_t* largest, hipStream_t s);
hipError_t launch_any_nodes(const AnyItem* items, const AnyWave* waves, const uint64_t* heads, uint32_t nwaves, uint32_t* node_off,
                            uint32_t* m_off, uint64_t* pos, uint8_t* flg, uint32_t* minc, uint32_t* midx, uint32_t* item,
                            hipStream_t s);
// ntot >= 1 nodes, sentinels included: the flat index and ok[item] = the item's chain holds its nseg segments
hipError_t launch_any_walk(const AnyItem* items, const uint64_t* heads, const AnyRange* range, const uint32_t* item,
                           const uint64_t* pos, const uint8_t* flg, const uint32_t* minc, const uint32_t* midx, uint32_t ntot,
                           uint32_t largest, uint32_t* nxt_a, uint32_t* nxt_b, uint8_t* lab, uint8_t* mark, uint32_t* lbl,
                           uint32_t* rank, uint32_t* tmp, uint32_t* total, uint64_t* index, uint32_t* ok, hipStream_t s);
// the items of one segment: index [b0, e], ok
hipError_t launch_any_single(const AnyItem* items, uint32_t nitems, const uint64_t* heads, uint64_t* index, uint32_t* ok,
                             hipStream_t s);
// behind the token stage, over a launch batch's segment table: depends[seg], and the strip rows of k_inflate_bytes (nseg slots,
// the unused ones empty).  An item's first segment (no history) always starts a row.
hipError_t launch_any_rows(const InflateSeg* segs, const SegInfo* info, const uint32_t* tokens, uint32_t nseg, uint8_t* depends,
                           uint32_t* starts, uint32_t* excl, uint32_t* tmp, uint32_t* nrows, InflateStrip* rows, hipStream_t s);
// recovered index (sfh_decompress_any*): the token kernels with the EXACT end rule for rows flagged kSegExact
hipError_t launch_inflate_tokens_exact(const InflateSeg* rows, uint32_t nseg, uint32_t* tokens, SegInfo* info, bool speculate,
                                       hipStream_t s);
// per item of the call: the wrapper (before the token kernels), then the status fold (behind every launch batch)
// (segs, sums: the call's segment and checksum rows, which a gzip item with ISIZE below its output size cuts down to ISIZE)
hipError_t launch_inflate_head(InflateItem* items, uint32_t nitems, uint32_t container, InflateSeg* segs, BatchChunk* sums,
                               hipStream_t s);
// first (nullable): per item, its first failing segment (0xFFFFFFFF: none)
hipError_t launch_inflate_fold(const InflateItem* items, uint32_t nitems, const SegInfo* info, const uint32_t* sums,
                               uint32_t container, uint32_t* status, uint32_t* first, hipStream_t s);
// items of one wide segment each (launch_bgzf_rows_wide): segment record seg0, checksum partials 2 * seg0 and 2 * seg0 + 1
hipError_t launch_inflate_fold_wide(const InflateItem* items, uint32_t nitems, const SegInfo* info, const uint32_t* sums,
                                    uint32_t container, uint32_t* status, hipStream_t s);
// random access: the byte stage with a write window per row, and every range's status (its span's first failing segment)
hipError_t launch_inflate_bytes_clip(const InflateSeg* rows, const InflateClip* clips, const InflateStrip* strips, uint32_t nstrips,
                                     const uint32_t* tokens, SegInfo* info, hipStream_t s);
hipError_t launch_inflate_fold_spans(const InflateSpan* spans, uint32_t nspans, const SegInfo* info, uint32_t* status, hipStream_t s);

// sf_stream.hip: streams without flush points (sfh_inflate_stream*, sfh_inflate_stream_batch*; a single stream is a call of one
// item); StreamChunk and the chain round: sf_stream_chain.h.  Every pass runs over the call's items, each read from a row.  The
// records of all items lie in one array, item after item; a record's item is a separate u32 (StreamChunk keeps its layout).
constexpr uint64_t kNoCandidate = ~0ull;
struct StreamItem {      // per item whose body is decoded (a wrapper that failed: no row)
  const uint8_t* src;
  uint64_t src_n;
  uint64_t b0, body_n;   // its body: bytes [b0, b0 + body_n) of src
  uint64_t plane;        // write pass: its first symbol-plane entry in its launch batch's plane
  uint64_t cap;          // write pass: its output capacity (gzip: ISIZE)
  uint8_t* dst;          // resolve: its output
  uint64_t win;          // compose / link / resolve: its first window entry in its launch batch's tables
  uint32_t c0;           // find: its first nominal chunk in the call (rows ascending by item)
  uint32_t r0, m;        // its records in the call's
  uint32_t chain, G;     // its confirmed records, and the chunks per group (stream_group(chain))
  uint32_t pad;
};
struct StreamGroup {     // compose / resolve: one workgroup per (item, group)
  uint32_t item, g;
};
static_assert(sizeof(StreamItem) == 88 && sizeof(StreamGroup) == 8, "stream item rows");
// one wave per nominal chunk of the call (nc), its item found by a search over items[].c0.  members: every item is a file of
// gzip members (b0: the first header's end, the body reaches to src_n), and a member's body start is a candidate too
hipError_t launch_stream_find(const StreamItem* items, uint32_t nitems, uint32_t nc, uint64_t step_bytes, uint64_t* cand,
                              hipStream_t s, bool members = false);
// list (nullable: 0..n-1): the records to decode; rec_item[r]: record r's row in items.  follow: one lane per list entry goes on
// into the records after it while their links break, within its item's records (see k_stream_decode).  write: the exact pass
// into plane + the item's offset.  side (null: no item is a file of gzip members; else every item is): the records' side rows,
// and mem, the write pass's member rows (sf_stream_chain.h)
hipError_t launch_stream_decode(bool write, const StreamItem* items, const uint32_t* rec_item, StreamChunk* recs,
                                const uint32_t* list, uint32_t n, bool follow, uint16_t* plane, hipStream_t s,
                                StreamSide* side = nullptr, StreamMember* mem = nullptr);
uint32_t stream_group(uint32_t n);  // chunks per group of the resolve; an item's tables: (groups - 1) * 32768 u16
// compose rows (every group but an item's last), link (one workgroup per item of more than one group), resolve rows (all)
hipError_t launch_stream_resolve(const uint16_t* plane, const StreamChunk* recs, const StreamItem* items,
                                 const StreamGroup* compose, uint32_t ncompose, const uint32_t* link, uint32_t nlink,
                                 const StreamGroup* resolve, uint32_t nresolve, uint16_t* tables, hipStream_t s);

// sf_zip.hip: ZIP archives (sf_zip_plan.h; sfh_zip_read_index_device, sfh_decompress_zip*, sfh_compress_zip*)
namespace zip {
struct Entry;
}
struct ZipCopy {         // per stored entry of a decode call
  const uint8_t* src;    // its data in the file (any alignment)
  uint8_t* dst;          // 16-byte aligned
  uint64_t n;
};
struct ZipPiece {        // per workgroup of a copy: 32 KiB piece `piece` of row `row`
  uint32_t row, piece;
};
struct ZipItem {         // per item of a compress call
  uint64_t name_off;     // its name in the names' bytes: the sum of the name lengths before it
  uint64_t slot_off;     // its raw stream's slot in the scratch of its launch batch (16-byte aligned), and the slot's bytes
  uint64_t slot_n;
  uint32_t name_len, usize;
};
static_assert(sizeof(ZipCopy) == 24 && sizeof(ZipPiece) == 8 && sizeof(ZipItem) == 32, "ZIP descriptor rows");
// one lane per entry: parse_local on the file's first `limit` bytes (the directory's first byte)
hipError_t launch_zip_locals(const uint8_t* src, uint64_t limit, zip::Entry* entries, uint64_t n, hipStream_t s);
// the stored entries' copy; file, file_n: what may be loaded around a source (the file up to its last byte's dword)
hipError_t launch_zip_store(const ZipCopy* rows, const ZipPiece* pieces, uint32_t npieces, const uint8_t* file, uint64_t file_n,
                            hipStream_t s);
// the writer, behind a launch batch of n items: off[i] = where item i's local header goes (*carry: the end of the batches before,
// moved on to this one's end); the pieces of the items' bounds, each copied as far as its stream reaches; and behind the last
// batch the directory, the end record(s) and *total
hipError_t launch_zip_place(const ZipItem* items, const uint64_t* out_n, uint32_t n, uint64_t* off, uint64_t* carry, hipStream_t s);
hipError_t launch_zip_pack(const ZipItem* items, const ZipPiece* pieces, uint32_t npieces, const uint8_t* names, const uint64_t* out_n,
                           const uint64_t* off, const uint32_t* crc, const uint8_t* slots, uint8_t* dst, hipStream_t s);
hipError_t launch_zip_wrap(const ZipItem* items, const uint8_t* names, const uint64_t* out_n, const uint64_t* off, const uint32_t* crc,
                           uint64_t n, uint64_t names_n, const uint64_t* carry, uint8_t* dst, uint64_t* total, hipStream_t s);

// sf_guard.hip: does the LDS execute a returning atomic's lanes in ascending order (op 0: ds_wrxchg_rtn_b32, 1: ds_mskor_rtn_b32)?
// d_result[0] = mismatches against the sequential model, [1] = positions checked
hipError_t run_lds_order_check(int op, uint32_t blocks, uint32_t iters, uint32_t* d_result, hipStream_t s);

uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);        // host arithmetic
uint32_t adler32_combine(uint32_t adler_a, uint32_t adler_b, uint64_t len_b);  // host arithmetic

}  // namespace sf
