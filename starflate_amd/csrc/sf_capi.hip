// sf_capi.hip -- the C-ABI of include/starflate_hip.h over the kernels of sf_kernels.hip.
// No torch types, no exceptions across the boundary.  A ctx owns its device scratch: every buffer, pinned block, event and stream
// below is a member that frees itself (sf_scratch.h), so sfh_destroy deletes the context and nothing else; one device buffer that
// holds several arrays is laid out with sf::stage::Carve (sf_stage_plan.h).  The compressor's workspace (sf::Workspace: the
// kernels' interface) stays raw pointers behind ensure_compress_ws / free_compress_ws, ensure_dtok and ensure_sums.
#include "../../include/starflate_hip.h"
#include "sf_any_plan.h"
#include "sf_bgzf_plan.h"
#include "sf_bgzf_range_plan.h"
#include "sf_device.h"
#include "sf_dz_plan.h"
#include "sf_inflate_core.h"
#include "sf_inflate_plan.h"
#include "sf_range_plan.h"
#include "sf_scratch.h"
#include "sf_stage_plan.h"
#include "sf_zip_plan.h"

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <thread>
#include <vector>

namespace {
using sf::scratch::Buf;
using sf::scratch::Event;
using sf::scratch::Pair;
using sf::scratch::Pinned;
using sf::scratch::Stager;
using sf::scratch::Stream;
using sf::stage::al16;
using sf::stage::Carve;
void free_compress_ws(sfh_ctx* c);
}  // namespace

struct sfh_ctx {
  int device = 0;
  Stream stream;                 // used when the caller passes no stream (declared first: destroyed behind every buffer and event)
  sf::Workspace ws{};
  uint32_t cap_chunks = 0;       // chunks of a call the compressor's index arrays (ws.offsets, ws.subidx) can hold
  uint32_t cap_batch = 0;        // chunks the compressor's batch arrays can hold
  uint32_t cap_dtok = 0;         // segments the decoder's token buffer can hold
  size_t seginfo_cap = 0;        // bytes of ws.seginfo
  size_t sums_cap = 0;           // bytes of ws.sums
  uint32_t last_chunks = 0;
  uint32_t last_block_bytes = 0; // strip size the last compress call used
  bool index_valid = false;      // ws.offsets holds the index of the last compress call
  Buf<uint64_t> d_total;         // own result slot for the synchronous entry points
  Pinned<uint64_t> h_total;      // ... and the pinned word it is copied to (a pageable target is staged by the runtime)
  Buf<uint32_t> d_value;         // result slot of sfh_checksum_device; [2] for the decoder's status
  Buf<sf::DzInfo> d_dzinfo;      // result slot of sfh_dz_read_index_device (on first use)
  // BGZF read (sfh_bgzf_read_index_device, sfh_decompress_bgzf_device), all on first use: the info slot; the scan's counts,
  // their scan and its scratch; the walk's node arrays; the decoder's own index; its rows, implied entries and statuses
  Buf<sf::BgzfInfo> d_bgzfinfo;
  Buf<uint32_t> d_bgzfcnt;
  Buf<uint8_t> d_bgzfwalk;
  Buf<uint64_t> d_bgzfix;
  Buf<uint8_t> d_bgzfrows;
  Buf<uint8_t> d_bgzfrng;        // sfh_decompress_bgzf_ranges*: the planner's per-range arrays (the rows: d_bgzfrows)
  Buf<uint64_t> d_index;         // staging for the host-buffer decoder
  Buf<uint32_t> d_sub;
  // per-stage events of the last profiled decode call: SFH_INFLATE_NSTAGES + 1 per batch, grown on demand
  std::vector<Event> ev_inf;
  uint32_t ev_inf_batches = 0;
  bool ev_inf_valid = false;
  size_t last_dtok_bytes = 0;    // bytes of decoder token scratch the last decode call used (bounded: one batch)
  Buf<uint8_t> d_in;             // staging for the host-buffer entry points: host_up, staged_up
  Buf<uint8_t> d_out;
  int profiling = 0;
  int k1_stamps = 0;  // SFH_K1_STAMPS=1: diagnostic k_lz77 build with s_memtime stamps
  uint32_t batch_chunks = sf::kBatchChunks;  // SFH_BATCH_CHUNKS=<n>: smaller batches (tests of the batch loop)
  // per-kernel events of the last profiled call: kEvPerBatch per batch (before k_lz77, k_plan, k_scan, k_emit and after
  // k_emit), then one after the container kernels; grown on demand, reused by later calls
  static constexpr int kEvPerBatch = 5;
  std::vector<Event> ev;
  uint32_t ev_batches = 0;       // batches the last profiled call recorded
  bool ev_valid = false;
  // host-buffer path (sfh_compress): copies of one batch run beside the kernels of its neighbours
  static constexpr int kPipe = 4;
  Stream s_in, s_out;
  Event ev_in[kPipe], ev_batch[kPipe];
  Pinned<uint64_t> h_tot;        // the stream's end after each batch in flight
  Event ev_done;                 // end of the last call's device work: the next call, on any stream, starts behind it
  bool busy = false;             // (the device scratch is shared by all calls on this ctx)
  hipStream_t last_stream = nullptr;
  Pair<uint64_t> sizes;          // sfh_gather_streams: the ranks' records on the device and in pinned memory
  int order_ok[2] = {0, 0};      // sfh_lds_order_check per op (0 exchange: chains, 1 masked-or: recent): 0 not run, 1 holds, -1 does not
  int force_order_fail = 0;      // SFH_FORCE_ORDER_FAIL=1: the library's own check reports failure (tests)
  int inflate_serial = 0;        // SFH_INFLATE_SERIAL=1: index-only streams through the lane-serial kernel alone (tests, A/B)
  // the batched calls' descriptor tables (compress or decompress), built in pinned memory and uploaded with one copy
  Stager tab{"pinned descriptor tables", "descriptor tables"};
  Pinned<uint8_t> h_stage;       // the batched host calls (staged_up, staged_down): pinned staging of the packed items (kStageBytes)
  Pair<uint64_t> bn;             // sfh_compress_batch: the items' sizes on the device and in pinned memory
  // the index of the last call when it was a compress batch (sfh_copy_batch_index): every item's entries, item after item, in
  // d_bix; the sub-index is ws.subidx (the call's chunks are the items' segments in order)
  bool bix_valid = false;
  Buf<uint64_t> d_bix;
  size_t bix_items = 0, bix_entries = 0;
  std::vector<uint32_t> bix_block_bytes;
  Buf<uint64_t> d_implied;       // sfh_decompress_batch* without an index: every item's two implied entries
  Pair<uint32_t> bstatus;        // sfh_decompress_batch: the statuses on the device and in pinned memory
  // decoding without side information (sfh_recover_index*, sfh_decompress_any* and their _batch calls): the per-wave counts of
  // the candidate scan, the node arrays of the walk, the recovered index and the per-segment arrays behind the token stage
  Buf<uint32_t> d_anycnt;
  Buf<uint8_t> d_any;
  Buf<uint8_t> d_anyseg;
  Buf<uint64_t> d_anyix;
  Buf<uint8_t> d_anyb;           // every item's body, node ranges and indexable flag; the totals
  Event ev_any[5];
  float any_ms[2] = {0, 0};
  uint64_t any_counts[2] = {0, 0};
  // streams without flush points (sfh_inflate_stream*, one item or a batch): candidates (then: the records' items | the follow
  // list) | chunk records | the redo list; the symbol plane; the composed windows of the resolve
  uint64_t stream_chunk = 16384;  // SFH_STREAM_CHUNK=<bytes>: nominal chunk size S
  Buf<uint8_t> d_stm;
  Buf<uint16_t> d_plane;
  Buf<uint16_t> d_wins;
  Event ev_stm[6];
  float stm_ms[SFH_STREAM_NSTAGES] = {};
  uint64_t stm_counts[SFH_STREAM_NCOUNTS] = {};
  // the wrapper rows and bodies | the item rows; a launch batch's group, checksum and fold rows and its statuses
  Buf<uint8_t> d_sbt;
  Buf<uint8_t> d_sbr;
  // files of gzip members (SFH_GZIP_MEMBERS): the write pass's member rows, and the last such call's table on the host
  // (SFH_DBG_STREAM_MEMBERS; valid until the next call of any kind ends)
  Buf<uint8_t> d_smem;
  std::vector<sf::StreamMember> stm_members;
  bool stm_members_valid = false;
  // ZIP (sfh_zip_read_index_device, sfh_decompress_zip*, sfh_compress_zip*), all on first use: the reader's tables (entry
  // table; copy, piece, checksum and fold rows and the statuses); the writer's tables, pinned and on the device (its own
  // stager: enqueue_zip's batch calls use `tab`), and the raw streams of one launch batch
  Buf<uint8_t> d_zip;
  Stager zipw{"pinned ZIP tables", "ZIP tables"};
  Buf<uint8_t> d_zipbody;
  char err[256] = {0};
  // the compressor's workspace and the decoder's three arrays in it are raw fields of ws (the kernels' interface)
  ~sfh_ctx() {
    free_compress_ws(this);
    (void)hipFree(ws.tokens);
    (void)hipFree(ws.seginfo);
    (void)hipFree(ws.sums);
  }
};

namespace {

int fail(sfh_ctx* c, int code, const char* what, hipError_t e) {
  if (c) snprintf(c->err, sizeof c->err, "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
  return code;
}

// the raw arrays of ws that are sized on their own (ensure_sums, ensure_seginfo): *p holds at least `bytes` afterwards
template <class T>
int grow_ws(sfh_ctx* ctx, T** p, size_t* cap_bytes, size_t bytes, const char* what) {
  if (*cap_bytes >= bytes) return SFH_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *cap_bytes = 0;
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return fail(ctx, SFH_E_NOMEM, what, e);
  *cap_bytes = bytes;
  return SFH_OK;
}

// the compressor's scratch; the decoder's (tokens, seginfo) and the checksum partials are sized on their own
void free_compress_ws(sfh_ctx* c) {
  (void)hipFree(c->ws.items);
  (void)hipFree(c->ws.nitems);
  (void)hipFree(c->ws.ntok);
  (void)hipFree(c->ws.hist);
  (void)hipFree(c->ws.plan);
  (void)hipFree(c->ws.codes);
  (void)hipFree(c->ws.ptree);
  (void)hipFree(c->ws.offsets);
  (void)hipFree(c->ws.stamps);
  (void)hipFree(c->ws.rtok);
  (void)hipFree(c->ws.subidx);
  const sf::Workspace keep = c->ws;
  c->ws = sf::Workspace{};
  c->ws.tokens = keep.tokens;
  c->ws.seginfo = keep.seginfo;
  c->ws.sums = keep.sums;
  c->cap_chunks = 0;
  c->cap_batch = 0;
}

// checksum partials: 4 bytes per chunk, needed without the rest of the workspace by sfh_checksum_device
int ensure_sums(sfh_ctx* ctx, uint32_t nchunks) {
  return grow_ws(ctx, &ctx->ws.sums, &ctx->sums_cap, (size_t)nchunks * sizeof(uint32_t), "checksum scratch");
}
// the decoders' segment records
int ensure_seginfo(sfh_ctx* ctx, size_t nseg) {
  return grow_ws(ctx, &ctx->ws.seginfo, &ctx->seginfo_cap, nseg * sizeof(sf::SegInfo), "segment records");
}

// The compressor's batch arrays hold min(nchunks, kBatchChunks) chunks, its index arrays (offsets, sub-index) every
// chunk of the call.
int ensure_compress_ws(sfh_ctx* ctx, uint32_t nchunks) {
  if (nchunks <= ctx->cap_chunks) return SFH_OK;
  free_compress_ws(ctx);
  // (a strip larger than a batch is its own batch: kMaxStrip / kChunk = 512 chunks at most)
  const size_t nc = nchunks, nb = std::min<uint32_t>(nchunks, std::max<uint32_t>(ctx->batch_chunks, sf::kMaxStrip / sf::kChunk));
  hipError_t e;
  if ((e = hipMalloc(&ctx->ws.items, nb * sf::kChunk * sizeof(uint16_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.nitems, nb * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.ntok, nb * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.hist, nb * sf::kHistStride * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.plan, nb * sizeof(sf::ChunkPlan))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.codes, nb * sizeof(sf::ChunkCodes))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.ptree, nb * sizeof(sf::PlanTree))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.rtok, nb * sf::kSubRegions * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.offsets, (nc + 1) * sizeof(uint64_t))) != hipSuccess ||
      (e = hipMalloc(&ctx->ws.subidx, nc * 2 * sf::kSubRegions * sizeof(uint32_t))) != hipSuccess) {
    free_compress_ws(ctx);
    return fail(ctx, SFH_E_NOMEM, "workspace hipMalloc", e);
  }
  if (ctx->k1_stamps && (e = hipMalloc(&ctx->ws.stamps, nb * 16 * sizeof(uint64_t))) != hipSuccess) {
    free_compress_ws(ctx);
    return fail(ctx, SFH_E_NOMEM, "stamps hipMalloc", e);
  }
  ctx->cap_chunks = nchunks;
  ctx->cap_batch = (uint32_t)nb;
  return SFH_OK;
}

// the decoder's token buffer (4 bytes per output byte) is only allocated once a decode call needs it
int ensure_dtok(sfh_ctx* ctx, uint32_t nseg) {
  if (nseg <= ctx->cap_dtok) return SFH_OK;
  (void)hipFree(ctx->ws.tokens);
  ctx->ws.tokens = nullptr;
  ctx->cap_dtok = 0;
  const hipError_t e = hipMalloc(&ctx->ws.tokens, (size_t)nseg * sf::kChunk * sizeof(uint32_t));
  if (e != hipSuccess) return fail(ctx, SFH_E_NOMEM, "decoder token buffer hipMalloc", e);
  ctx->cap_dtok = nseg;
  return SFH_OK;
}

uint32_t chunks_of(size_t n) { return n ? (uint32_t)((n + sf::kChunk - 1) / sf::kChunk) : 1u; }
// the bytes of a stream in front of its trailer (zlib: Adler-32, gzip: CRC-32 and ISIZE): where its DEFLATE body ends at the latest
inline uint64_t body_bytes(uint32_t container, uint64_t src_n) {
  const uint64_t trailer = container == SFH_ZLIB ? 4 : container == SFH_GZIP ? 8 : 0;
  return src_n > trailer ? src_n - trailer : 0;
}

// block_bytes = 0: SFH_DEFAULT_BLOCK_BYTES -- larger (SFH_LARGE_BLOCK_BYTES, SFH_CHAIN_BLOCK_BYTES with a chain effort)
// while the input still fills the device four times over with such strips (a strip starts with an empty window: fewer
// starts, a better ratio, the same time per byte), smaller while it has fewer than 256 strips.  A function of n and the
// effort alone, so the stream is too (the encoder specification states the same rule)
uint32_t resolve_block_bytes(uint32_t block_bytes, size_t n, uint32_t effort = SFH_EFFORT_DEFAULT) {
  if (block_bytes) return block_bytes;
  const bool chain = effort >= SFH_EFFORT_BEST && effort <= SFH_EFFORT_EXTREME;
  uint32_t b = chain ? SFH_CHAIN_BLOCK_BYTES : SFH_LARGE_BLOCK_BYTES;
  while (b > SFH_DEFAULT_BLOCK_BYTES && n / b < (chain ? 1024u : 2048u)) b >>= 1;
  while (b > sf::kChunk && n / b < 256) b >>= 1;
  return b;
}

// Calls on one ctx share its device scratch: a call enqueued on another stream than the previous one first waits
// (on the device) for that one's work.
int order_behind_last_call(sfh_ctx* ctx, hipStream_t s) {
  if (ctx->busy && ctx->last_stream != s) SF_HIP(hipStreamWaitEvent(s, ctx->ev_done, 0), "wait for the previous call");
  return SFH_OK;
}
int mark_call_end(sfh_ctx* ctx, hipStream_t s) {
  SF_HIP(hipEventRecord(ctx->ev_done, s), "event");
  ctx->busy = true;
  ctx->last_stream = s;
  ctx->stm_members_valid = false;
  return SFH_OK;
}
// What opens a device entry point: the context's device is current, whatever launch error an earlier caller on this thread
// left is dropped (launches are checked with hipGetLastError()), and *s is the caller's stream, or the context's for none.
int begin_call(sfh_ctx* ctx, void* stream, hipStream_t* s) {
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();
  *s = stream ? (hipStream_t)stream : ctx->stream;
  return SFH_OK;
}
// A host-buffer call begins on an idle context: EVERY one of them waits here, on the host, for the last call's device work.
// It fills the context's staging (d_in, d_index, d_sub; h_stage) with copies on the context's stream that are issued before
// its device path takes its place behind the last call (order_behind_last_call), and that call -- on a caller's stream, or
// one that returned an error with work in flight -- may still use the staging (sfh_decompress_dz_device on a caller's stream
// decodes from d_index).  After a call that ended synchronised the event has fired and this returns at once.
int wait_idle(sfh_ctx* ctx) {
  if (ctx->busy) SF_HIP(hipEventSynchronize(ctx->ev_done), "wait for the last call");
  return SFH_OK;
}
// the timing events of a profiled call, grown on demand: `v` holds at least `need` afterwards
int ensure_events(sfh_ctx* ctx, std::vector<Event>& v, size_t need) {
  while (v.size() < need) {
    Event e;
    SF_HIP(hipEventCreate(&e.h), "event");
    v.push_back(std::move(e));
  }
  return SFH_OK;
}

// dictzip: the caller writes SFH_DICTZIP (the single-stream calls; enqueue() checks what that container asks beyond this)
int check_opt(const sfh_options* o, bool dictzip = false) {
  if (!o) return 0;
  if (o->strategy > SFH_DYNAMIC || o->final_stream > 1 || o->lazy > 3 || o->no_stored_fast_path > 1) return -1;
  if (o->container > (dictzip ? SFH_DICTZIP : SFH_GZIP) || (o->container && !o->final_stream)) return -1;  // a non-final shard has no trailer
  if (o->block_bytes % sf::kChunk || o->block_bytes > sf::kMaxStrip) return -1;
  if (o->effort > SFH_EFFORT_RECENT_ALL || o->chain_depth > 255) return -1;
  if (o->chain_depth && (o->effort < SFH_EFFORT_BEST || o->effort > SFH_EFFORT_EXTREME)) return -1;
  return 0;
}

// The returning LDS atomic of the exact-recency match finders (op 0: chains, op 1: recent) executes a wave's lanes in
// ascending order on this device?  Checked once per context IN sfh_create, on the context's own stream (64 workgroups x 4
// steps x 5 densities: 1.2 M positions, well under a millisecond of kernels), so that no compress call -- an asynchronous
// one on the caller's stream, possibly under capture -- ever launches or waits for it; ensure_order() reads the verdict
// (and runs the check itself only if sfh_create could not).
int check_order(sfh_ctx* ctx, int op, uint64_t* bad, uint64_t* checked, uint32_t blocks, uint32_t iters) {
  SF_HIP(sf::run_lds_order_check(op, blocks, iters, ctx->d_value, ctx->stream), "lds order check");
  uint32_t r[2] = {0, 0};
  SF_HIP(hipMemcpyAsync(r, ctx->d_value, sizeof r, hipMemcpyDeviceToHost, ctx->stream), "lds order check result");
  SF_HIP(hipStreamSynchronize(ctx->stream), "lds order check sync");
  *bad = r[0];
  *checked = r[1];
  return SFH_OK;
}
int ensure_order(sfh_ctx* ctx, int op) {
  if (ctx->order_ok[op] == 0) {
    uint64_t bad = 0, checked = 0;
    const int rc = check_order(ctx, op, &bad, &checked, 64, 4);
    if (rc) return rc;
    ctx->order_ok[op] = (bad == 0 && checked != 0 && !ctx->force_order_fail) ? 1 : -1;
  }
  if (ctx->order_ok[op] < 0) {
    snprintf(ctx->err, sizeof ctx->err, "%s does not execute a wave's lanes in ascending order on this device%s: the %s need it",
             op ? "ds_mskor_rtn_b32" : "ds_wrxchg_rtn_b32", ctx->force_order_fail ? " (SFH_FORCE_ORDER_FAIL=1)" : "",
             op ? "effort SFH_EFFORT_RECENT" : "chain efforts (SFH_EFFORT_BEST / _ULTRA / _EXTREME)");
    return SFH_E_UNSUPPORTED;
  }
  return SFH_OK;
}

// Host buffers of sfh_compress: with them the batch loop also moves the data -- batch b's input goes up on one copy
// stream while batch b-1 is in the kernels and batch b-2's stream bytes go down on another.
struct HostPipe {
  const uint8_t* src;
  uint8_t* dst;
  size_t cap;
  size_t copied = 0;   // stream bytes already on their way to dst
  bool overflow = false;
};
constexpr uint32_t kPipeBatchChunks = 2048;  // 64 MiB of input per batch on the host-buffer path
constexpr size_t kStageBytes = (size_t)kPipeBatchChunks * sf::kChunk;  // the pinned staging (h_stage) of the batched host calls

// effort -> what the match kernel does: {both levels, near candidate, even positions only, second table, chain depth, exact recency}
sf::Options kernel_options(const sfh_options& o, uint32_t strip_bytes) {
  const uint32_t ef = o.effort;
  const bool ef_chain = ef >= SFH_EFFORT_BEST && ef <= SFH_EFFORT_EXTREME, ef_recent = ef == SFH_EFFORT_RECENT || ef == SFH_EFFORT_RECENT_ALL;
  const bool ef_all = ef == SFH_EFFORT_THOROUGH || ef == SFH_EFFORT_MAX || ef_chain || ef == SFH_EFFORT_RECENT_ALL;  // every position searched
  return sf::Options{o.strategy, o.final_stream, o.lazy, o.no_stored_fast_path ? 0u : (o.strategy == 0 ? 2u : 1u),
                     strip_bytes,
                     (ef == SFH_EFFORT_FAST || ef == SFH_EFFORT_FASTEST) ? 0u : 1u,
                     ef == SFH_EFFORT_FASTEST ? 0u : 1u, ef_all ? 0u : 1u,
                     ef == SFH_EFFORT_MAX ? 1u : 0u,
                     !ef_chain ? 0u : o.chain_depth ? o.chain_depth
                     : ef == SFH_EFFORT_BEST ? 8u : ef == SFH_EFFORT_ULTRA ? 16u : 32u,
                     ef_recent ? 1u : 0u};
}

// bgzf (sfh_compress_bgzf*): the raw stream at block_bytes = 32768 with every chunk closed (BFINAL) and wrapped as a gzip
// member of its own -- k_scan leaves 26 bytes around every block, k_bgzf_wrap fills them in behind each launch batch -- and
// the EOF member behind the last.  Off: nothing below differs from before.
int enqueue(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap, uint64_t* d_out_n,
            const sfh_options* opt, hipStream_t s, HostPipe* pipe = nullptr, bool bgzf = false) {
  if (!ctx || (!d_src && n) || !d_dst || !d_out_n || check_opt(opt, true)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 3)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 16, dst 4)", hipSuccess);
  sfh_options o;
  if (opt) o = *opt; else sfh_default_options(&o);
  if (bgzf) {
    if (o.container != SFH_RAW || o.final_stream != 1 || (o.block_bytes && o.block_bytes != sf::kChunk))
      return fail(ctx, SFH_E_INVALID_ARG, "BGZF: container SFH_RAW, final_stream 1, block_bytes 0 or 32768", hipSuccess);
    o.block_bytes = sf::kChunk;
    if (cap < sfh_bgzf_bound(n)) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_bgzf_bound(n)", hipSuccess);
  }
  // SFH_DICTZIP: the gzip stream at block_bytes = 32768 (the table promises independent chunks), its header with the table
  const bool dictzip = o.container == SFH_DICTZIP;
  if (dictzip) {
    if ((o.block_bytes && o.block_bytes != sf::kChunk) || n > sf::dz::kMaxInput)
      return fail(ctx, SFH_E_INVALID_ARG, "SFH_DICTZIP: block_bytes 0 or 32768, n <= SFH_DZ_MAX_CHUNKS * 32768", hipSuccess);
    o.block_bytes = sf::kChunk;
    o.container = SFH_GZIP;
    if (cap < sfh_compress_bound_container(n, sf::kChunk, SFH_DICTZIP))
      return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_compress_bound_container(n)", hipSuccess);
  }
  if (cap < sfh_compress_bound(n, 0)) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_compress_bound(n)", hipSuccess);
  if (n > ((size_t)1 << 44)) return fail(ctx, SFH_E_INVALID_ARG, "input too large", hipSuccess);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();  // launches are checked with hipGetLastError(): drop whatever an earlier caller on this thread left
  const uint32_t nchunks = chunks_of(n);
  int rc = ensure_compress_ws(ctx, nchunks);
  if (!rc && (o.container || bgzf)) rc = ensure_sums(ctx, nchunks);
  if (rc) return rc;
  ctx->last_chunks = nchunks;
  ctx->bix_valid = false;
  sf::Options ko = kernel_options(o, resolve_block_bytes(o.block_bytes, n, o.effort));
  if (bgzf) ko.final_stream = 2;  // every chunk ends its own stream (plan_chunk)
  if ((ko.chain_depth || ko.recent) && (rc = ensure_order(ctx, ko.recent ? 1 : 0)) != SFH_OK) return rc;
  ctx->last_block_bytes = ko.strip_bytes;
  const bool prof = ctx->profiling != 0;
  if ((rc = order_behind_last_call(ctx, s)) != SFH_OK) return rc;
  // Batches of whole strips, at most kBatchChunks chunks each, one after the other on the stream: strips are coded
  // independently, so the stream is the same as from one launch over everything.  (Per-kernel events: the first batch.)
  const uint32_t per_strip = ko.strip_bytes / sf::kChunk;
  const uint32_t want = pipe ? std::min(ctx->batch_chunks, kPipeBatchChunks) : ctx->batch_chunks;
  const uint32_t batch = std::max(per_strip, want / per_strip * per_strip);
  const uint32_t nbatches = (nchunks + batch - 1) / batch;
  ctx->ev_valid = false;
  if (prof && (rc = ensure_events(ctx, ctx->ev, (size_t)nbatches * sfh_ctx::kEvPerBatch + 1)) != SFH_OK) return rc;
  const size_t hdr = sf::wrapper_header_bytes(o.container, dictzip ? nchunks : 0u);
  if (pipe) pipe->copied = hdr;  // the wrapper header is written last (k_wrap) and copied last
  if (bgzf && n == 0) {  // the EOF member alone
    ctx->ev_valid = false;
    ctx->index_valid = false;
    SF_HIP(sf::launch_bgzf_wrap(nullptr, nullptr, 0, 0, (uint8_t*)d_dst, d_out_n, 2u, s), "launch k_bgzf_wrap");
    return mark_call_end(ctx, s);
  }
  // the stream bytes of batch `b` (its end is in h_tot once ev_batch fires) go down while later batches run
  auto drain = [&](uint32_t b) -> int {
    SF_HIP(hipEventSynchronize(ctx->ev_batch[b % sfh_ctx::kPipe]), "wait for a batch");
    const size_t end = (size_t)ctx->h_tot[b % sfh_ctx::kPipe];
    if (end > pipe->cap) { pipe->overflow = true; return SFH_OK; }
    if (end > pipe->copied)
      SF_HIP(hipMemcpyAsync(pipe->dst + pipe->copied, (const uint8_t*)d_dst + pipe->copied, end - pipe->copied,
                            hipMemcpyDeviceToHost, ctx->s_out), "D2H");
    pipe->copied = end;
    return SFH_OK;
  };
  uint32_t bi = 0;
  for (uint32_t c0 = 0; c0 < nchunks; c0 += batch, ++bi) {
    const uint32_t nb = std::min(batch, nchunks - c0);
    const bool first = c0 == 0, last = c0 + nb == nchunks;
    const uint8_t* bsrc = (const uint8_t*)d_src + (size_t)c0 * sf::kChunk;
    const size_t bn = std::min((size_t)nb * sf::kChunk, n - (size_t)c0 * sf::kChunk);
    if (pipe && bn) {
      SF_HIP(hipMemcpyAsync(const_cast<uint8_t*>(bsrc), pipe->src + (size_t)c0 * sf::kChunk, bn, hipMemcpyHostToDevice, ctx->s_in), "H2D");
      SF_HIP(hipEventRecord(ctx->ev_in[bi % sfh_ctx::kPipe], ctx->s_in), "event");
      SF_HIP(hipStreamWaitEvent(s, ctx->ev_in[bi % sfh_ctx::kPipe], 0), "wait for the input");
    }
    sf::Workspace w = ctx->ws;  // this batch's view: index arrays advance, batch arrays start over
    w.offsets += c0;
    w.subidx += (size_t)c0 * 2 * sf::kSubRegions;
    sf::Options bo = ko;
    bo.final_stream = (last || bgzf) ? ko.final_stream : 0u;
    // every batch has its own events (recorded behind the wait for its input, so a kernel's time excludes the copy)
    Event* ev = prof ? &ctx->ev[(size_t)bi * sfh_ctx::kEvPerBatch] : nullptr;
    if (ev) SF_HIP(hipEventRecord(ev[0], s), "event");
    SF_HIP(sf::launch_lz77(bsrc, bn, nb, w, bo, s), "launch k_lz77");
    if (ev) SF_HIP(hipEventRecord(ev[1], s), "event");
    SF_HIP(sf::launch_plan(bn, nb, w, bo, s), "launch k_plan");
    if (ev) SF_HIP(hipEventRecord(ev[2], s), "event");
    SF_HIP(sf::launch_scan(nb, w, hdr, !first, d_out_n, s, nullptr, bgzf ? sf::bgzf::kHeader : 0u, bgzf ? sf::bgzf::kWrap : 0u),
           "launch k_scan");
    if (ev) SF_HIP(hipEventRecord(ev[3], s), "event");
    SF_HIP(sf::launch_emit(bsrc, bn, nb, w, bo, (uint8_t*)d_dst, s), "launch k_emit");
    if (ev) SF_HIP(hipEventRecord(ev[4], s), "event");
    if (bgzf) {  // the batch's members are complete before its bytes are drained; the last batch's lane 0 appends the EOF member
      SF_HIP(sf::launch_checksum(bsrc, bn, nb, SFH_GZIP, ctx->ws.sums + c0, s), "launch k_checksum");
      SF_HIP(sf::launch_bgzf_wrap(ctx->ws.sums + c0, w.offsets, nb, bn, (uint8_t*)d_dst, d_out_n, last ? 1u : 0u, s), "launch k_bgzf_wrap");
    }
    if (pipe) {
      if (bi >= 1 && (rc = drain(bi - 1)) != SFH_OK) return rc;  // (its slot is free again before batch bi + kPipe - 1 needs it)
      SF_HIP(hipMemcpyAsync(&ctx->h_tot[bi % sfh_ctx::kPipe], d_out_n, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy size");
      SF_HIP(hipEventRecord(ctx->ev_batch[bi % sfh_ctx::kPipe], s), "event");
    }
  }
  if (pipe && (rc = drain(bi - 1)) != SFH_OK) return rc;
  if (o.container) {
    SF_HIP(sf::launch_checksum((const uint8_t*)d_src, n, nchunks, o.container, ctx->ws.sums, s), "launch k_checksum");
    // (dictzip: the table is the differences of the call's index, complete behind the last batch's k_scan)
    SF_HIP(sf::launch_wrap(ctx->ws.sums, nchunks, n, o.container, (uint8_t*)d_dst, d_out_n, nullptr, s, dictzip ? ctx->ws.offsets : nullptr),
           "launch k_wrap");
  }
  if (prof) {
    SF_HIP(hipEventRecord(ctx->ev[(size_t)nbatches * sfh_ctx::kEvPerBatch], s), "event");
    ctx->ev_batches = nbatches;
  }
  ctx->ev_valid = prof;
  ctx->index_valid = !bgzf;  // (BGZF: the offsets are the blocks' inside their members, no index of a stream)
  return mark_call_end(ctx, s);
}

// Destinations must not overlap: sorted by address, each ends before the next begins.  (A destination of no bytes is written
// nothing and overlaps nothing: it is left out.)
int check_disjoint(sfh_ctx* ctx, void* const* dsts, const uint64_t* lens, size_t count) {
  std::vector<size_t> ord;
  try {
    ord.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  size_t m = 0;
  for (size_t i = 0; i < count; ++i)
    if (lens[i]) ord[m++] = i;
  std::sort(ord.begin(), ord.begin() + (std::ptrdiff_t)m, [&](size_t a, size_t b) { return (uintptr_t)dsts[a] < (uintptr_t)dsts[b]; });
  for (size_t k = 1; k < m; ++k)
    if ((uintptr_t)dsts[ord[k - 1]] + lens[ord[k - 1]] > (uintptr_t)dsts[ord[k]])
      return fail(ctx, SFH_E_INVALID_ARG, "destination ranges overlap", hipSuccess);
  return SFH_OK;
}

// the per-stage events of a profiled decode call: SFH_INFLATE_NSTAGES + 1 per launch batch
int ensure_inflate_events(sfh_ctx* ctx, uint32_t nbatches) {
  return ensure_events(ctx, ctx->ev_inf, (size_t)nbatches * (SFH_INFLATE_NSTAGES + 1));
}

// ---- batched compression (sfh_compress_batch*) ----
// Everything a batch call checks before it enqueues anything (`dev`: device buffers, the single call's alignment rules).
int check_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, void* const* dsts,
                const uint64_t* dst_cap, const void* out_n, const sfh_options* opt, bool dev) {
  if (!ctx || check_opt(opt)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (count == 0) return SFH_OK;
  if (!srcs || !src_n || !dsts || !dst_cap || !out_n) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many items", hipSuccess);
  uint64_t chunks = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((!srcs[i] && src_n[i]) || !dsts[i]) return fail(ctx, SFH_E_INVALID_ARG, "null item pointer", hipSuccess);
    if (dev && (((uintptr_t)srcs[i] & 15) || ((uintptr_t)dsts[i] & 3)))
      return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 16, dst 4)", hipSuccess);
    if (src_n[i] > ((uint64_t)1 << 44)) return fail(ctx, SFH_E_INVALID_ARG, "item too large", hipSuccess);
    if (dst_cap[i] < sfh_compress_bound((size_t)src_n[i], 0)) return fail(ctx, SFH_E_DST_TOO_SMALL, "dst_cap < sfh_compress_bound(n)", hipSuccess);
    chunks += chunks_of((size_t)src_n[i]);
  }
  if (chunks > ((uint64_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 chunks in one call", hipSuccess);
  return check_disjoint(ctx, dsts, dst_cap, count);  // (no capacity is 0: sfh_compress_bound > 0)
}

// One launch batch: its rows in the call's tables (chunk rows are the call's, in item order; strip and item rows per batch).
struct LaunchBatch {
  uint32_t c0 = 0, nchunks = 0, s0 = 0, nstrips = 0, i0 = 0, nitems = 0;
};

// Device buffers, arguments checked (check_batch).  The host builds the descriptor tables -- per strip, per chunk, per item
// of a launch batch, and with a container per item of the call -- and uploads them in one copy; then every launch batch
// runs k_lz77 .. k_emit over its rows, and with a container k_checksum / k_wrap run once over the call's rows.
// crc_partials (raw items; sfh_compress_zip*): k_checksum leaves the CRC-32 partial of every chunk of the call in ws.sums, in
// item order, and no wrapper is written.
int enqueue_batch(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, void* const* d_dsts,
                  uint64_t* d_out_n, const sfh_options* opt, hipStream_t s, bool crc_partials = false) {
  sfh_options o;
  if (opt) o = *opt; else sfh_default_options(&o);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();  // see enqueue()
  std::vector<sf::BatchStrip> strips;
  std::vector<sf::BatchChunk> chunks;
  std::vector<sf::BatchItem> items;
  std::vector<sf::WrapItem> wraps;
  std::vector<sf::BatchIndexRow> ixrows;
  std::vector<LaunchBatch> lbs;
  const uint32_t cap = ctx->batch_chunks;
  try {
    ctx->bix_block_bytes.resize(count);
    LaunchBatch cur;
    auto close = [&] {
      if (cur.nchunks) lbs.push_back(cur);
      cur = LaunchBatch{};
      cur.c0 = (uint32_t)chunks.size();
      cur.s0 = (uint32_t)strips.size();
      cur.i0 = (uint32_t)items.size();
    };
    // chunks [k0, k1) of item i (whole strips of it, k0 on a strip boundary) into the current launch batch
    auto add = [&](size_t i, uint32_t strip_bytes, uint32_t k0, uint32_t k1, uint32_t nc) {
      const uint8_t* src = (const uint8_t*)d_srcs[i];
      const uint64_t n = src_n[i];
      const uint32_t per = strip_bytes / sf::kChunk, it = cur.nitems++;
      items.push_back(sf::BatchItem{(uint8_t*)d_dsts[i], 0, (uint32_t)i, cur.nchunks, k1 - k0, k0 ? 1u : 0u});
      for (uint32_t k = k0; k < k1; k += per) {
        const uint64_t b = (uint64_t)k * sf::kChunk;
        strips.push_back(sf::BatchStrip{src + b, (uint32_t)std::min<uint64_t>(strip_bytes, n - b), cur.nchunks + (k - k0)});
        ++cur.nstrips;
      }
      for (uint32_t k = k0; k < k1; ++k) {
        const uint64_t b = (uint64_t)k * sf::kChunk;
        chunks.push_back(sf::BatchChunk{src + b, (uint32_t)std::min<uint64_t>(sf::kChunk, n - b), it << 1 | (k + 1 == nc ? 1u : 0u)});
        ixrows.push_back(sf::BatchIndexRow{(uint32_t)items.size() - 1, (uint32_t)i});
      }
      cur.nchunks += k1 - k0;
    };
    close();
    for (size_t i = 0; i < count; ++i) {
      const uint32_t sb = resolve_block_bytes(o.block_bytes, (size_t)src_n[i], o.effort), per = sb / sf::kChunk;
      const uint32_t nc = chunks_of((size_t)src_n[i]);
      ctx->bix_block_bytes[i] = sb;
      if (o.container) wraps.push_back(sf::WrapItem{(uint8_t*)d_dsts[i], src_n[i], (uint32_t)i, (uint32_t)chunks.size(), nc, 0});
      if (nc <= cap) {  // whole, in the current launch batch or the next
        if (cur.nchunks + nc > cap) close();
        add(i, sb, 0, nc, nc);
        continue;
      }
      // larger than a launch batch: batches of its own, cut at its strips as the single call cuts them (its stream carries on)
      close();
      const uint32_t piece = std::max(per, cap / per * per);
      for (uint32_t k0 = 0; k0 < nc; k0 += piece) {
        add(i, sb, k0, std::min(nc, k0 + piece), nc);
        close();
      }
    }
    close();
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the descriptor tables", hipSuccess);
  }
  const uint32_t nchunks = (uint32_t)chunks.size();
  // the batch arrays hold the widest launch batch (at most a batch or a strip: ensure_compress_ws), the index arrays the call
  ctx->bix_valid = false;
  int rc = ensure_compress_ws(ctx, nchunks);
  if (!rc && (o.container || crc_partials)) rc = ensure_sums(ctx, nchunks);
  if (!rc) rc = ctx->d_bix.grow(ctx, (size_t)nchunks + count, "batch index");
  if (rc) return rc;
  const sf::Options ko = kernel_options(o, sf::kChunk);  // (strip_bytes: the strip table's)
  if ((ko.chain_depth || ko.recent) && (rc = ensure_order(ctx, ko.recent ? 1 : 0)) != SFH_OK) return rc;
  // the tables, in one pinned block: chunks | strips | items | wraps | index rows
  Carve L;
  const size_t o_chunks = L.add<sf::BatchChunk>(chunks.size()), o_strips = L.add<sf::BatchStrip>(strips.size());
  const size_t o_items = L.add<sf::BatchItem>(items.size()), o_wraps = L.add<sf::WrapItem>(wraps.size());
  const size_t o_ixrows = L.add<sf::BatchIndexRow>(ixrows.size()), bytes = L.bytes();
  if ((rc = ctx->tab.stage(ctx, bytes)) != SFH_OK) return rc;
  memcpy(ctx->tab.h + o_chunks, chunks.data(), chunks.size() * sizeof(sf::BatchChunk));
  memcpy(ctx->tab.h + o_strips, strips.data(), strips.size() * sizeof(sf::BatchStrip));
  memcpy(ctx->tab.h + o_items, items.data(), items.size() * sizeof(sf::BatchItem));
  memcpy(ctx->tab.h + o_wraps, wraps.data(), wraps.size() * sizeof(sf::WrapItem));
  memcpy(ctx->tab.h + o_ixrows, ixrows.data(), ixrows.size() * sizeof(sf::BatchIndexRow));
  const sf::BatchChunk* d_chunks = Carve::at<const sf::BatchChunk>(ctx->tab.d, o_chunks);
  const sf::BatchStrip* d_strips = Carve::at<const sf::BatchStrip>(ctx->tab.d, o_strips);
  sf::BatchItem* d_items = Carve::at<sf::BatchItem>(ctx->tab.d, o_items);
  const sf::WrapItem* d_wraps = Carve::at<const sf::WrapItem>(ctx->tab.d, o_wraps);
  const sf::BatchIndexRow* d_ixrows = Carve::at<const sf::BatchIndexRow>(ctx->tab.d, o_ixrows);

  ctx->index_valid = false;  // a batch has no single index: the index functions refuse until the next single call
  ctx->last_chunks = lbs.back().nchunks;
  const bool prof = ctx->profiling != 0;
  if ((rc = ctx->tab.upload(ctx, bytes, s)) != SFH_OK) return rc;
  const uint32_t nbatches = (uint32_t)lbs.size();
  ctx->ev_valid = false;
  if (prof && (rc = ensure_events(ctx, ctx->ev, (size_t)nbatches * sfh_ctx::kEvPerBatch + 1)) != SFH_OK) return rc;
  const uint64_t hdr = sf::wrapper_header_bytes(o.container);
  for (uint32_t bi = 0; bi < nbatches; ++bi) {
    const LaunchBatch& b = lbs[bi];
    const sf::BatchTables bt{d_strips + b.s0, b.nstrips, d_chunks + b.c0, d_items + b.i0, b.nitems};
    sf::Workspace w = ctx->ws;  // k_scan's offsets and k_emit's sub-index land at the batch's places in the call's index arrays
    w.offsets += b.c0;
    w.subidx += (size_t)b.c0 * 2 * sf::kSubRegions;
    Event* ev = prof ? &ctx->ev[(size_t)bi * sfh_ctx::kEvPerBatch] : nullptr;
    if (ev) SF_HIP(hipEventRecord(ev[0], s), "event");
    SF_HIP(sf::launch_lz77(nullptr, 0, b.nchunks, ctx->ws, ko, s, &bt), "launch k_lz77");
    if (ev) SF_HIP(hipEventRecord(ev[1], s), "event");
    SF_HIP(sf::launch_plan(0, b.nchunks, ctx->ws, ko, s, &bt), "launch k_plan");
    if (ev) SF_HIP(hipEventRecord(ev[2], s), "event");
    SF_HIP(sf::launch_scan(b.nchunks, w, hdr, false, d_out_n, s, &bt), "launch k_scan");
    if (ev) SF_HIP(hipEventRecord(ev[3], s), "event");
    SF_HIP(sf::launch_emit(nullptr, 0, b.nchunks, w, ko, nullptr, s, &bt), "launch k_emit");
    if (ev) SF_HIP(hipEventRecord(ev[4], s), "event");
  }
  // (behind the launch batches and ahead of k_wrap_batch: d_out_n is still every stream's end before its trailer)
  SF_HIP(sf::launch_batch_index(d_chunks, d_ixrows, d_items, ctx->ws.offsets, d_out_n, nchunks, ctx->d_bix, s), "launch k_batch_index");
  if (crc_partials) SF_HIP(sf::launch_checksum_batch(d_chunks, nchunks, SFH_GZIP, ctx->ws.sums, s), "launch k_checksum");
  if (o.container) {
    SF_HIP(sf::launch_checksum_batch(d_chunks, nchunks, o.container, ctx->ws.sums, s), "launch k_checksum");
    SF_HIP(sf::launch_wrap_batch(ctx->ws.sums, d_wraps, (uint32_t)count, o.container, d_out_n, s), "launch k_wrap");
  }
  if (prof) {
    SF_HIP(hipEventRecord(ctx->ev[(size_t)nbatches * sfh_ctx::kEvPerBatch], s), "event");
    ctx->ev_batches = nbatches;
  }
  ctx->ev_valid = prof;
  ctx->bix_valid = true;
  ctx->bix_items = count;
  ctx->bix_entries = (size_t)nchunks + count;
  return mark_call_end(ctx, s);
}

// ---- batched decompression (sfh_decompress_batch*) ----
// Everything the call checks before it enqueues anything (`dev`: device buffers, the single decoder's alignment rules).
int check_inflate_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, const uint64_t* index,
                        const uint32_t* subindex, void* const* dsts, const uint64_t* dst_n, const uint32_t* block_bytes,
                        uint32_t container, const uint32_t* status, bool dev) {
  if (!ctx || container > SFH_GZIP) return fail(ctx, SFH_E_INVALID_ARG, "argument (container)", hipSuccess);
  if (count == 0) return SFH_OK;
  if (!srcs || !src_n || !dsts || !dst_n || !status) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many items", hipSuccess);
  if (subindex && !index) return fail(ctx, SFH_E_INVALID_ARG, "a sub-index without an index", hipSuccess);
  if (dev && (((uintptr_t)index & 7) || ((uintptr_t)subindex & 3) || ((uintptr_t)status & 3)))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (index 8, sub-index 4, status 4)", hipSuccess);
  uint64_t segs = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((!srcs[i] && src_n[i]) || (!dsts[i] && dst_n[i])) return fail(ctx, SFH_E_INVALID_ARG, "null item pointer", hipSuccess);
    if (dev && (((uintptr_t)srcs[i] & 3) || ((uintptr_t)dsts[i] & 15)))
      return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
    if (dst_n[i] > ((uint64_t)1 << 44)) return fail(ctx, SFH_E_INVALID_ARG, "item too large", hipSuccess);
    const uint32_t bb = block_bytes ? block_bytes[i] : 0u;
    if (bb % sf::kChunk || bb > sf::kMaxStrip)
      return fail(ctx, SFH_E_INVALID_ARG, "block_bytes: a multiple of 32768 up to 16 MiB (0 = 32768)", hipSuccess);
    if (!index && dst_n[i] > sf::kChunk) return fail(ctx, SFH_E_INVALID_ARG, "no index, and an item above 32768 bytes", hipSuccess);
    segs += chunks_of((size_t)dst_n[i]);
  }
  if (segs > ((uint64_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 segments in one call", hipSuccess);
  return check_disjoint(ctx, dsts, dst_n, count);
}

// Device buffers, arguments checked.  The launch batches are planned (sf_inflate_plan.h: whole items, an item larger than a
// batch in batches of its own at its strips), which also says how large the tables are; the host then writes them straight into
// the pinned block -- per segment, per strip, per item, and with a container per checksum chunk -- uploads them in one copy,
// and then: k_inflate_head (wrappers, implied index entries), the token and byte kernels batch after batch,
// k_checksum_batch over the decoded bytes and k_inflate_fold (every item's status; d_first, nullable: its first failing segment).
int enqueue_inflate_batch(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, const uint64_t* d_index,
                          const uint32_t* d_subindex, void* const* d_dsts, const uint64_t* dst_n, const uint32_t* block_bytes,
                          uint32_t container, uint32_t* d_status, uint32_t* d_first, hipStream_t s) {
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();  // see enqueue()
  int rc = SFH_OK;
  if (!d_index && (rc = ctx->d_implied.grow(ctx, 2 * count, "implied index"))) return rc;
  sf::iplan::Plan P;
  try {
    sf::iplan::plan_batches(count, dst_n, block_bytes, ctx->batch_chunks, P);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the launch batches", hipSuccess);
  }
  const uint32_t nseg = P.nseg;
  rc = ensure_seginfo(ctx, (size_t)nseg);
  if (!rc) rc = ensure_dtok(ctx, P.widest);
  if (!rc && container) rc = ensure_sums(ctx, nseg);
  if (rc) return rc;
  // the tables, in one pinned block: segments | items | strips | checksum chunks
  Carve L;
  const size_t o_segs = L.add<sf::InflateSeg>(nseg), o_items = L.add<sf::InflateItem>(count), o_strips = L.add<sf::InflateStrip>(P.nstrips);
  const size_t o_sums = L.add<sf::BatchChunk>(container ? nseg : 0), bytes = L.bytes();
  if ((rc = ctx->tab.stage(ctx, bytes)) != SFH_OK) return rc;
  sf::InflateSeg* h_segs = Carve::at<sf::InflateSeg>(ctx->tab.h, o_segs);
  sf::InflateItem* h_items = Carve::at<sf::InflateItem>(ctx->tab.h, o_items);
  sf::InflateStrip* h_strips = Carve::at<sf::InflateStrip>(ctx->tab.h, o_strips);
  sf::BatchChunk* h_sums = Carve::at<sf::BatchChunk>(ctx->tab.h, o_sums);
  uint32_t seg0 = 0;  // the item's first segment in the call; its first index entry: the items before have one more each
  for (size_t i = 0; i < count; ++i) {
    const uint32_t n = sf::iplan::segments_of(dst_n[i]);
    h_items[i] = sf::InflateItem{(const uint8_t*)d_srcs[i], src_n[i], dst_n[i], d_index ? nullptr : ctx->d_implied + 2 * i,
                                 d_index ? d_index + seg0 + i : nullptr, seg0, n, 0, 0, 0, 0};
    seg0 += n;
  }
  uint32_t g = 0, t = 0;  // the next segment and strip row (the batches follow each other in both tables)
  for (const sf::iplan::Batch& b : P.batches)
    sf::iplan::for_rows(
        b, dst_n, block_bytes, [&](uint32_t first, uint32_t n) { h_strips[t++] = sf::InflateStrip{first, n}; },
        [&](size_t i, uint32_t k) {
          // (segment g of the call is entry g + i of the flattened index: every item before this one has an entry more than segments)
          const uint64_t* ix = d_index ? d_index + (g + i) : ctx->d_implied + 2 * i;
          uint8_t* out = (uint8_t*)d_dsts[i] + (uint64_t)k * sf::kChunk;
          const uint32_t on = sf::iplan::seg_out_n(dst_n[i], k);
          const uint64_t body_n = body_bytes(container, src_n[i]);
          // (the segments are the call's in item order: the flattened sub-index holds segment g at g * SFH_SUBINDEX_WORDS)
          h_segs[g] = sf::InflateSeg{(const uint8_t*)d_srcs[i], ix, d_subindex ? d_subindex + (size_t)g * SFH_SUBINDEX_WORDS : nullptr,
                                     out, body_n, on,
                                     sf::iplan::seg_hist(k, sf::iplan::sps_of(block_bytes, i)) | (container ? sf::kSegWrapped : 0u)};
          if (container) h_sums[g] = sf::BatchChunk{out, on, 0u};
          ++g;
        });
  sf::InflateSeg* t_segs = Carve::at<sf::InflateSeg>(ctx->tab.d, o_segs);
  sf::InflateItem* t_items = Carve::at<sf::InflateItem>(ctx->tab.d, o_items);
  const sf::InflateStrip* t_strips = Carve::at<const sf::InflateStrip>(ctx->tab.d, o_strips);
  sf::BatchChunk* t_sums = Carve::at<sf::BatchChunk>(ctx->tab.d, o_sums);

  ctx->index_valid = false;  // the last call is now this one: what sfh_debug_read returns belongs to it
  ctx->bix_valid = false;
  ctx->last_chunks = nseg;
  ctx->last_dtok_bytes = (size_t)P.widest * sf::kChunk * sizeof(uint32_t);
  const bool prof = ctx->profiling != 0;
  if ((rc = ctx->tab.upload(ctx, bytes, s)) != SFH_OK) return rc;
  const uint32_t nbatches = (uint32_t)P.batches.size();
  ctx->ev_inf_valid = false;
  if (prof && (rc = ensure_inflate_events(ctx, nbatches)) != SFH_OK) return rc;
  SF_HIP(sf::launch_inflate_head(t_items, (uint32_t)count, container, t_segs, container ? t_sums : nullptr, s), "launch k_inflate_head");
  // The token scratch (4 bytes per output byte) holds ONE batch -- 4 GiB for any size of call -- and the two stages alternate
  // on the stream, batch after batch.  Strips decode independently, the segment records and the statuses cover the whole call,
  // so the result -- bytes, first failing segment, its status -- is that of one pass over everything.
  for (uint32_t bi = 0; bi < nbatches; ++bi) {
    const sf::iplan::Batch& b = P.batches[bi];
    sf::SegInfo* binfo = ctx->ws.seginfo + b.row0;
    Event* ev = prof ? &ctx->ev_inf[(size_t)bi * (SFH_INFLATE_NSTAGES + 1)] : nullptr;
    if (ev) SF_HIP(hipEventRecord(ev[0], s), "event");
    SF_HIP(sf::launch_inflate_tokens(t_segs + b.row0, b.nseg, ctx->ws.tokens, binfo, d_subindex != nullptr, !ctx->inflate_serial, s),
           "launch k_inflate_tokens");
    if (ev) SF_HIP(hipEventRecord(ev[1], s), "event");
    SF_HIP(sf::launch_inflate_bytes(t_segs + b.row0, t_strips + b.strip0, b.nstrips, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes");
    if (ev) SF_HIP(hipEventRecord(ev[2], s), "event");
  }
  ctx->ev_inf_batches = nbatches;
  ctx->ev_inf_valid = prof;
  if (container) SF_HIP(sf::launch_checksum_batch(t_sums, nseg, container, ctx->ws.sums, s), "launch k_checksum");
  SF_HIP(sf::launch_inflate_fold(t_items, (uint32_t)count, ctx->ws.seginfo, ctx->ws.sums, container, d_status, d_first, s),
         "launch k_inflate_fold");
  return mark_call_end(ctx, s);
}

// ---- random access (sfh_decompress_range*) ----
// Everything the call checks before it plans or enqueues anything (`dev`: device buffers, the decoder's alignment rules; dsts
// are free of them).
int check_ranges(sfh_ctx* ctx, const void* src, const uint64_t* index, const uint32_t* subindex, size_t nseg, uint64_t total_n,
                 uint32_t block_bytes, size_t count, const uint64_t* offsets, const uint64_t* lengths, void* const* dsts,
                 const uint32_t* status, bool dev) {
  if (!ctx) return fail(ctx, SFH_E_INVALID_ARG, "argument (context)", hipSuccess);
  if (count == 0) return SFH_OK;
  if (!src || !index || !offsets || !lengths || !dsts || !status) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many ranges", hipSuccess);
  if (total_n > sf::range::kMaxTotal || nseg != (size_t)sf::range::segments_of(total_n))
    return fail(ctx, SFH_E_INVALID_ARG, "nseg != max(1, ceil(total_n / 32768))", hipSuccess);
  if (block_bytes % sf::kChunk || block_bytes > sf::kMaxStrip)
    return fail(ctx, SFH_E_INVALID_ARG, "block_bytes: a multiple of 32768 up to 16 MiB (0 = 32768)", hipSuccess);
  if (dev && (((uintptr_t)src & 3) || ((uintptr_t)index & 7) || ((uintptr_t)subindex & 3) || ((uintptr_t)status & 3)))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, index 8, sub-index 4, status 4)", hipSuccess);
  for (size_t r = 0; r < count; ++r) {
    if (!dsts[r] && lengths[r]) return fail(ctx, SFH_E_INVALID_ARG, "null destination", hipSuccess);
    if (offsets[r] > total_n || lengths[r] > total_n - offsets[r])
      return fail(ctx, SFH_E_INVALID_ARG, "a range ends behind total_n", hipSuccess);
  }
  return check_disjoint(ctx, dsts, lengths, count);
}

int plan_ranges_checked(sfh_ctx* ctx, uint64_t total_n, uint32_t block_bytes, size_t count, const uint64_t* offsets,
                        const uint64_t* lengths, sf::range::Plan& P) {
  try {
    const int pr = sf::range::plan_ranges(total_n, block_bytes, count, offsets, lengths, ctx->batch_chunks, P);
    if (pr == sf::range::kPlanTooMany)
      return fail(ctx, SFH_E_INVALID_ARG, "decode spans of more than 2^31 - 1 segments in one call", hipSuccess);
    if (pr) return fail(ctx, SFH_E_INVALID_ARG, "argument (ranges)", hipSuccess);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the range plan", hipSuccess);
  }
  return SFH_OK;
}

// What the rows of one range's decode span read: the stream base its index entries are offsets into and the bytes readable
// from it, the index entry and (or null) the sub-index words of the span's FIRST segment -- the later rows' follow.
struct RangeSource {
  const uint8_t* src;
  uint64_t src_n;
  const uint64_t* ix;
  const uint32_t* sub;
};

// Device buffers, arguments checked, the plan made.  The host builds the tables -- per row its InflateSeg and its write
// window, per strip, per range its span -- and uploads them in one copy; then the token kernels (as they are, over the rows)
// and the clipped byte stage batch after batch, and the fold of every range's status.
int enqueue_ranges(sfh_ctx* ctx, const sf::range::Plan& P, const RangeSource* from, void* const* d_dsts, size_t count, bool sub,
                   uint32_t* d_status, hipStream_t s) {
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();  // see enqueue()
  const size_t nrows = P.rows.size(), nstrips = P.strips.size();
  Carve L;  // segments | write windows | strips | spans
  const size_t o_segs = L.add<sf::InflateSeg>(nrows), o_clips = L.add<sf::InflateClip>(nrows);
  const size_t o_strips = L.add<sf::InflateStrip>(nstrips), o_spans = L.add<sf::InflateSpan>(count), bytes = L.bytes();
  int rc = ensure_seginfo(ctx, nrows);
  if (!rc) rc = ensure_dtok(ctx, P.widest);
  if (!rc) rc = ctx->tab.stage(ctx, bytes);
  if (rc) return rc;
  sf::InflateSeg* h_segs = Carve::at<sf::InflateSeg>(ctx->tab.h, o_segs);
  sf::InflateClip* h_clips = Carve::at<sf::InflateClip>(ctx->tab.h, o_clips);
  sf::InflateStrip* h_strips = Carve::at<sf::InflateStrip>(ctx->tab.h, o_strips);
  sf::InflateSpan* h_spans = Carve::at<sf::InflateSpan>(ctx->tab.h, o_spans);
  for (size_t g = 0; g < nrows; ++g) {
    const sf::range::Row& w = P.rows[g];
    const RangeSource& f = from[w.range];
    const size_t k = g - P.spans[w.range].row0;
    h_segs[g] = sf::InflateSeg{f.src, f.ix + k, sub ? f.sub + k * SFH_SUBINDEX_WORDS : nullptr, nullptr, f.src_n, w.out_n, w.hist};
    h_clips[g] = sf::InflateClip{(uint8_t*)d_dsts[w.range] + w.dst_off, w.lo, w.hi};
  }
  for (size_t k = 0; k < nstrips; ++k) h_strips[k] = sf::InflateStrip{P.strips[k].row0, P.strips[k].nrows};
  for (size_t r = 0; r < count; ++r) h_spans[r] = sf::InflateSpan{P.spans[r].row0, P.spans[r].nrows};
  const sf::InflateSeg* t_segs = Carve::at<const sf::InflateSeg>(ctx->tab.d, o_segs);
  const sf::InflateClip* t_clips = Carve::at<const sf::InflateClip>(ctx->tab.d, o_clips);
  const sf::InflateStrip* t_strips = Carve::at<const sf::InflateStrip>(ctx->tab.d, o_strips);
  const sf::InflateSpan* t_spans = Carve::at<const sf::InflateSpan>(ctx->tab.d, o_spans);

  ctx->index_valid = false;
  ctx->bix_valid = false;
  ctx->last_chunks = (uint32_t)nrows;
  ctx->last_dtok_bytes = (size_t)P.widest * sf::kChunk * sizeof(uint32_t);
  const bool prof = ctx->profiling != 0;
  if ((rc = ctx->tab.upload(ctx, bytes, s)) != SFH_OK) return rc;
  const uint32_t nbatches = (uint32_t)P.batches.size();
  ctx->ev_inf_valid = false;
  if (prof && (rc = ensure_inflate_events(ctx, nbatches)) != SFH_OK) return rc;
  for (uint32_t bi = 0; bi < nbatches; ++bi) {
    const sf::range::Batch& b = P.batches[bi];
    sf::SegInfo* binfo = ctx->ws.seginfo + b.row0;
    Event* ev = prof ? &ctx->ev_inf[(size_t)bi * (SFH_INFLATE_NSTAGES + 1)] : nullptr;
    if (ev) SF_HIP(hipEventRecord(ev[0], s), "event");
    SF_HIP(sf::launch_inflate_tokens(t_segs + b.row0, b.nrows, ctx->ws.tokens, binfo, sub, !ctx->inflate_serial, s),
           "launch k_inflate_tokens");
    if (ev) SF_HIP(hipEventRecord(ev[1], s), "event");
    SF_HIP(sf::launch_inflate_bytes_clip(t_segs + b.row0, t_clips + b.row0, t_strips + b.strip0, b.nstrips, ctx->ws.tokens, binfo, s),
           "launch k_inflate_bytes_clip");
    if (ev) SF_HIP(hipEventRecord(ev[2], s), "event");
  }
  ctx->ev_inf_batches = nbatches;
  ctx->ev_inf_valid = prof;
  SF_HIP(sf::launch_inflate_fold_spans(t_spans, (uint32_t)count, ctx->ws.seginfo, d_status, s), "launch k_inflate_fold_spans");
  return mark_call_end(ctx, s);
}

// ---- the host-buffer entry points' staging ("one staging path") ----
// Pieces of a packed layout (sf_stage_plan.h) between the callers' buffers and the device, through the pinned h_stage: piece i
// lies at [off[i], off[i] + len[i]) of `total` bytes at d_base (up) or ctx->d_out (down); one copy and one wait per
// kStageBytes.  Down, len[i] == 0 skips piece i, and a stretch of kStageBytes that holds no other piece's bytes is not copied.
int stage_up(sfh_ctx* ctx, void* d_base, const void* const* srcs, const uint64_t* len, const uint64_t* off, size_t count,
             uint64_t total, hipStream_t s) {
  return sf::stage::pack_up(ctx->h_stage, kStageBytes, srcs, len, off, count, total, [&](uint64_t p0, uint64_t n) -> int {
    SF_HIP(hipMemcpyAsync((uint8_t*)d_base + p0, ctx->h_stage, n, hipMemcpyHostToDevice, s), "H2D");
    SF_HIP(hipStreamSynchronize(s), "stream sync");  // (the next piece refills h_stage)
    return SFH_OK;
  });
}
int stage_down(sfh_ctx* ctx, void* const* dsts, const uint64_t* len, const uint64_t* off, size_t count, uint64_t total,
               hipStream_t s) {
  return sf::stage::unpack_down(ctx->h_stage, kStageBytes, dsts, len, off, count, total, [&](uint64_t p0, uint64_t n) -> int {
    SF_HIP(hipMemcpyAsync(ctx->h_stage, ctx->d_out + p0, n, hipMemcpyDeviceToHost, s), "D2H");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    return SFH_OK;
  });
}

// A batched host-buffer call, on the context's stream: check, staged_up, the device path over d_srcs / d_dsts, the statuses,
// staged_down.  The items lie packed in ctx->d_in at in_off, their output slots in ctx->d_out at out_off.
struct Staged {
  std::vector<uint64_t> in_off, out_off, got;  // count + 1 offsets each; got: what staged_down copies of every item
  std::vector<const void*> d_srcs;
  std::vector<void*> d_dsts;
};
// Up: the layout, the device staging for it, the pinned buffer, an idle context (wait_idle), and the items go up.  slot: the
// bytes of ctx->d_out each item's output may take; null: the call has no output there, or lays it out later itself
// (stream_batch_run, into out_off).
int staged_up(sfh_ctx* ctx, Staged& B, size_t count, const void* const* srcs, const uint64_t* src_n, const uint64_t* slot) {
  try {
    B.in_off.resize(count + 1);
    B.got.resize(count);
    B.d_srcs.resize(count);
    if (slot) B.out_off.resize(count + 1);
    if (slot) B.d_dsts.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  sf::stage::pack_layout(src_n, count, B.in_off.data());
  if (slot) sf::stage::pack_layout(slot, count, B.out_off.data());
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = ctx->d_in.grow(ctx, std::max<uint64_t>(16, B.in_off[count]), "input staging");
  if (!rc && slot) rc = ctx->d_out.grow(ctx, std::max<uint64_t>(16, B.out_off[count]), "output staging");
  if (!rc) rc = ctx->h_stage.grow(ctx, kStageBytes, "pinned staging");
  if (!rc) rc = wait_idle(ctx);
  if (rc) return rc;
  if ((rc = stage_up(ctx, ctx->d_in, srcs, src_n, B.in_off.data(), count, B.in_off[count], ctx->stream))) return rc;
  for (size_t i = 0; i < count; ++i) {
    B.d_srcs[i] = ctx->d_in + B.in_off[i];
    if (slot) B.d_dsts[i] = ctx->d_out + B.out_off[i];
  }
  return SFH_OK;
}
// Down: n[i] bytes of item i's slot to dsts[i] -- of the items that have a destination and (status given) status 0.  Nothing is
// written to any other item's, and nothing behind the last copied item's end comes down.
int staged_down(sfh_ctx* ctx, Staged& B, size_t count, void* const* dsts, const uint64_t* n, const uint32_t* status) {
  uint64_t end = 0;
  for (size_t i = 0; i < count; ++i) {
    B.got[i] = (dsts[i] && !(status && status[i])) ? n[i] : 0;
    if (B.got[i]) end = B.out_off[i] + B.got[i];
  }
  return stage_down(ctx, dsts, B.got.data(), B.out_off.data(), count, end, ctx->stream);
}

// The single-item host calls: no layout and no pinned buffer -- src goes up to ctx->d_in with one copy from the caller's buffer
// (d_out sized for out_n bytes), on an idle context as above; host_down fetches d_out[0, n) into dst and synchronises.
int host_up(sfh_ctx* ctx, const void* src, size_t src_n, size_t out_n) {
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = ctx->d_in.grow(ctx, std::max<size_t>(16, src_n), "input staging");
  if (!rc) rc = ctx->d_out.grow(ctx, std::max<size_t>(16, out_n), "output staging");
  if (!rc) rc = wait_idle(ctx);
  if (rc) return rc;
  if (src_n) SF_HIP(hipMemcpyAsync(ctx->d_in, src, src_n, hipMemcpyHostToDevice, ctx->stream), "H2D");
  return SFH_OK;
}
int host_down(sfh_ctx* ctx, void* dst, size_t n) {
  if (!n) return SFH_OK;
  SF_HIP(hipMemcpyAsync(dst, ctx->d_out, n, hipMemcpyDeviceToHost, ctx->stream), "D2H");
  SF_HIP(hipStreamSynchronize(ctx->stream), "stream sync");
  return SFH_OK;
}

// bstatus.d / bstatus.h hold `count` statuses; read_bstatus: the call's, behind its device path (synchronises s)
int ensure_bstatus(sfh_ctx* ctx, size_t count) { return ctx->bstatus.grow(ctx, count, "batch statuses"); }
int read_bstatus(sfh_ctx* ctx, size_t count, uint32_t* status, hipStream_t s) {
  SF_HIP(hipMemcpyAsync(ctx->bstatus.h, ctx->bstatus.d, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "copy statuses");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  memcpy(status, ctx->bstatus.h, count * sizeof(uint32_t));
  return SFH_OK;
}

// The indexed decoder's answer for a batch of one: its status and first failing segment (k_inflate_fold wrote them to
// d_value[0..1]) -> *status, and the message.  Synchronises s.
int read_decode_status(sfh_ctx* ctx, uint32_t* status, hipStream_t s) {
  uint32_t res[2] = {0, 0};
  SF_HIP(hipMemcpyAsync(res, ctx->d_value, sizeof res, hipMemcpyDeviceToHost, s), "copy status");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *status = res[0];
  if (res[0]) snprintf(ctx->err, sizeof ctx->err, "segment %u: DecompressStatus %u", res[1], res[0]);
  return SFH_OK;
}

// gzip's ISIZE, for SFH_SIZE_FROM_TRAILER on host buffers (a stream too short for a trailer: 0, and the device, which reads the
// wrapper, says what is wrong with it)
uint64_t trailer_isize(const void* src, uint64_t src_n) {
  const uint8_t* p = (const uint8_t*)src;
  return src_n >= 18 ? (uint64_t)(p[src_n - 4] | (uint32_t)p[src_n - 3] << 8 | (uint32_t)p[src_n - 2] << 16 | (uint32_t)p[src_n - 1] << 24) : 0;
}

// ---- decoding without side information (sfh_recover_index*, sfh_decompress_any*, and their _batch calls) ----
// One driver: a single stream is a call of one item.
constexpr uint32_t kStDstTooSmall = 4;  // the reference's DecompressStatus::DstTooSmall

// Everything a call checks before it enqueues anything (`dev`: device buffers, the single call's alignment rules).  dsts /
// dst_cap null: sfh_recover_index_batch* (dst_n are sizes, d_index the flat index).
int check_any_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                    void* const* dsts, const uint64_t* dst_cap, const uint64_t* dst_n, const uint64_t* index, bool recover,
                    const uint32_t* status, bool dev) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if (container > SFH_GZIP) return fail(ctx, SFH_E_INVALID_ARG, "argument (container)", hipSuccess);
  if (count == 0) return SFH_OK;
  if (!srcs || !src_n || !dst_n || !status || (recover ? !index : (!dsts || !dst_cap)))
    return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many items", hipSuccess);
  if (dev && recover && ((uintptr_t)index & 7)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (index 8)", hipSuccess);
  uint64_t segs = 0, waves = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((!srcs[i] && src_n[i]) || (!recover && !dsts[i] && dst_cap[i])) return fail(ctx, SFH_E_INVALID_ARG, "null item pointer", hipSuccess);
    if (dev && (((uintptr_t)srcs[i] & 3) || (!recover && ((uintptr_t)dsts[i] & 15))))
      return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
    const bool trailer = dst_n[i] == SFH_SIZE_FROM_TRAILER;
    if (trailer && (container != SFH_GZIP || recover))
      return fail(ctx, SFH_E_INVALID_ARG, "SFH_SIZE_FROM_TRAILER: a gzip stream of a decode call only", hipSuccess);
    if (src_n[i] > ((uint64_t)1 << 44) || (!trailer && dst_n[i] > ((uint64_t)1 << 44)) || (!recover && dst_cap[i] > ((uint64_t)1 << 44)))
      return fail(ctx, SFH_E_INVALID_ARG, "item too large (sizes up to 2^44)", hipSuccess);
    // (ISIZE is 32 bits wide, and one above the capacity is refused for the item)
    const uint64_t n = trailer ? std::min<uint64_t>(dst_cap[i], 0xFFFFFFFFu) : (!recover && dst_n[i] > dst_cap[i]) ? 0 : dst_n[i];
    const uint32_t ns = chunks_of((size_t)n);
    segs += ns;
    if (ns > 1) waves += (src_n[i] + 8191) / 8192;
  }
  if (segs > ((uint64_t)1 << 31) - 1 || waves > ((uint64_t)1 << 31) - 1)
    return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 segments or scan waves in one call", hipSuccess);
  return recover ? SFH_OK : check_disjoint(ctx, dsts, dst_cap, count);
}

// what the recovery leaves on the host, per item of the call
struct AnyBatch {
  std::vector<uint64_t> out_n;  // the size the item decodes to (SFH_SIZE_FROM_TRAILER resolved; 0 where the wrapper failed)
  std::vector<uint64_t> ix0;    // its first entry in the flat index
  std::vector<uint32_t> st;     // 0: indexable; the wrapper's status, DstTooSmall, or SFH_ITEM_NOT_INDEXABLE
  std::vector<uint8_t> take;    // st == 0
  uint64_t entries = 0;         // of the flat index
};

// d_anyb: heads u64[2 count] | ranges AnyRange[count] | ok u32[count] | totals u32[8] (nodes, M nodes, labels, -, -, largest)
// The recovery of a whole call: the wrappers (k_inflate_head over every item), one scan over every item that has more than one
// segment, one walk over the concatenated node lists.  d_index: the flat index (zeroed first: the entries of an item that is
// not indexable stay 0).  Synchronises s: after the wrappers only where ISIZE sizes the work, after the node count, after the
// walk.  Arguments checked (check_any_batch; the single calls: check_any, check_any_waves).
// bodies (raw items only; null: an item's body is all of it): every item's body [b0, e) inside its src_n bytes, two entries per
// item, host memory that outlives the call's first synchronisation -- a ZIP entry's data inside the 4-byte aligned item around it.
int any_batch_recover(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                      const uint64_t* dst_cap, const uint64_t* dst_n, uint64_t* d_index, hipStream_t s, AnyBatch& R,
                      const uint64_t* bodies = nullptr) {
  const bool prof = ctx->profiling != 0;
  ctx->any_ms[0] = ctx->any_ms[1] = 0;
  ctx->any_counts[0] = ctx->any_counts[1] = 0;
  std::vector<sf::InflateItem> rows;
  std::vector<sf::AnyItem> items;
  std::vector<uint32_t> okv;
  bool trailer = false;
  try {
    R.out_n.assign(count, 0);
    R.ix0.assign(count, 0);
    R.st.assign(count, 0);
    R.take.assign(count, 0);
    rows.resize(count);
    items.resize(count);
    okv.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (Event& e : ctx->ev_any)
    if (!e) SF_HIP(hipEventCreate(&e.h), "event");
  Carve A;
  const size_t o_heads = A.add<uint64_t>(2 * count), o_rng = A.add<sf::AnyRange>(count), o_ok = A.add<uint32_t>(count), o_tot = A.add<uint32_t>(8);
  int rc = ctx->d_anyb.grow(ctx, A.bytes(), "recovery tables");
  if (rc) return rc;
  uint64_t* heads = Carve::at<uint64_t>(ctx->d_anyb, o_heads);
  sf::AnyRange* range = Carve::at<sf::AnyRange>(ctx->d_anyb, o_rng);
  uint32_t* ok = Carve::at<uint32_t>(ctx->d_anyb, o_ok);
  uint32_t* tot = Carve::at<uint32_t>(ctx->d_anyb, o_tot);
  for (size_t i = 0; i < count; ++i) {
    const bool tr = dst_n[i] == SFH_SIZE_FROM_TRAILER;
    trailer |= tr;
    // an explicit size above the capacity: the item takes no part (an empty row: the wrapper check reads nothing of it)
    if (!tr && dst_cap && dst_n[i] > dst_cap[i]) R.st[i] = kStDstTooSmall;
    // (a size from the trailer: k_inflate_head's own ISIZE check, against the capacity)
    rows[i] = sf::InflateItem{(const uint8_t*)d_srcs[i], src_n[i], tr ? dst_cap[i] : dst_n[i], heads + 2 * i, nullptr, 0, 0, 0, 0, 0, 0};
    R.out_n[i] = tr ? 0 : dst_n[i];
  }
  // the item rows, the scan's item rows and its wave map: one pinned block, uploaded at once -- or, where ISIZE sizes the work,
  // the item rows first and the rest once the wrappers are read
  uint64_t segs = 0, nw = 0;
  auto geometry = [&] {
    segs = nw = 0;
    for (size_t i = 0; i < count; ++i) {
      const uint32_t ns = R.st[i] ? 1u : chunks_of((size_t)R.out_n[i]);
      const uint32_t w = (ns > 1 && !R.st[i]) ? sf::any_scan_waves(src_n[i]) : 0u;
      R.ix0[i] = segs + i;
      items[i] = sf::AnyItem{(const uint8_t*)d_srcs[i], src_n[i], R.ix0[i], ns, (uint32_t)nw, w, 0};
      segs += ns;
      nw += w;
    }
    R.entries = segs + count;
  };
  // the scan's rows behind what L holds already: added, the block staged, the rows filled in
  Carve L;
  size_t o_items = 0, o_waves = 0;
  auto stage_scan_rows = [&]() -> int {
    o_items = L.add<sf::AnyItem>(count);
    o_waves = L.add<sf::AnyWave>((size_t)nw);
    if (int e = ctx->tab.stage(ctx, L.bytes())) return e;
    memcpy(ctx->tab.h + o_items, items.data(), count * sizeof(sf::AnyItem));
    sf::AnyWave* wv = Carve::at<sf::AnyWave>(ctx->tab.h, o_waves);
    for (size_t i = 0; i < count; ++i)
      for (uint32_t p = 0; p < items[i].nwaves; ++p) wv[items[i].wave0 + p] = sf::AnyWave{(uint32_t)i, p};
    return SFH_OK;
  };
  const size_t b_rows = count * sizeof(sf::InflateItem);
  if (!trailer) {
    geometry();
    L.add<sf::InflateItem>(count);  // (the item rows: at 0)
    if ((rc = stage_scan_rows()) != SFH_OK) return rc;
    memcpy(ctx->tab.h, rows.data(), b_rows);
    if ((rc = ctx->tab.upload(ctx, L.bytes(), s)) != SFH_OK) return rc;
    SF_HIP(sf::launch_inflate_head(Carve::at<sf::InflateItem>(ctx->tab.d, 0), (uint32_t)count, container, nullptr, nullptr, s), "launch k_inflate_head");
    if (bodies) SF_HIP(hipMemcpyAsync(heads, bodies, 16 * count, hipMemcpyHostToDevice, s), "H2D bodies");  // (over the implied ones)
  } else {
    if ((rc = ctx->tab.stage(ctx, b_rows)) != SFH_OK) return rc;
    memcpy(ctx->tab.h, rows.data(), b_rows);
    if ((rc = ctx->tab.upload(ctx, b_rows, s)) != SFH_OK) return rc;
    SF_HIP(sf::launch_inflate_head(Carve::at<sf::InflateItem>(ctx->tab.d, 0), (uint32_t)count, container, nullptr, nullptr, s), "launch k_inflate_head");
    SF_HIP(hipMemcpyAsync(rows.data(), ctx->tab.d, b_rows, hipMemcpyDeviceToHost, s), "D2H wrapper rows");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    for (size_t i = 0; i < count; ++i) {
      if (!R.st[i] && rows[i].wst) R.st[i] = rows[i].wst;
      if (dst_n[i] == SFH_SIZE_FROM_TRAILER) R.out_n[i] = rows[i].wst ? 0 : rows[i].isize;
    }
    geometry();
    if (segs > ((uint64_t)1 << 31) - 1 || nw > ((uint64_t)1 << 31) - 1)
      return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 segments or scan waves in one call", hipSuccess);
    if ((rc = stage_scan_rows()) != SFH_OK) return rc;
    if ((rc = ctx->tab.upload(ctx, L.bytes(), s)) != SFH_OK) return rc;
  }
  const sf::AnyItem* t_items = Carve::at<const sf::AnyItem>(ctx->tab.d, o_items);
  const sf::AnyWave* t_waves = Carve::at<const sf::AnyWave>(ctx->tab.d, o_waves);
  if (!d_index) {
    if ((rc = ctx->d_anyix.grow(ctx, R.entries, "recovered index"))) return rc;
    d_index = ctx->d_anyix;
  }
  SF_HIP(hipMemsetAsync(d_index, 0, R.entries * sizeof(uint64_t), s), "clear the index");
  SF_HIP(hipMemsetAsync(ok, 0, A.bytes() - o_ok, s), "clear the flags");
  SF_HIP(sf::launch_any_single(t_items, (uint32_t)count, heads, d_index, ok, s), "launch k_any_single");
  const uint32_t nwaves = (uint32_t)nw;
  if (nwaves) {
    const size_t tw = sf::any_scan_tmp_words(nwaves);
    if ((rc = ctx->d_anycnt.grow(ctx, 2 * (size_t)nwaves + tw, "candidate counts"))) return rc;
    uint32_t* cn = ctx->d_anycnt;
    uint32_t* cm = cn + nwaves;
    uint32_t* tmp = cm + nwaves;
    if (prof) SF_HIP(hipEventRecord(ctx->ev_any[0], s), "event");
    SF_HIP(sf::launch_any_count(t_items, t_waves, heads, nwaves, cn, cm, s), "launch k_any_scan");
    SF_HIP(sf::launch_scan_u32(cn, cn, nwaves, tmp, tot + 0, s), "launch scan");
    SF_HIP(sf::launch_scan_u32(cm, cm, nwaves, tmp, tot + 1, s), "launch scan");
    SF_HIP(sf::launch_any_ranges(t_items, (uint32_t)count, cn, cm, nwaves, tot, range, tot + 5, s), "launch k_any_ranges");
    if (prof) SF_HIP(hipEventRecord(ctx->ev_any[1], s), "event");
    uint32_t h[6] = {0, 0, 0, 0, 0, 0};
    SF_HIP(hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, s), "D2H node count");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    const uint32_t n = h[0], nm = h[1], largest = h[5];  // n: sentinels included, one per item that was scanned
    uint32_t scanned = 0;
    for (size_t i = 0; i < count; ++i) scanned += items[i].nwaves ? 1u : 0u;
    ctx->any_counts[0] = n - scanned;
    // pos u64[n] | nxt_a, nxt_b, minc, lbl, rank, item u32[n] | midx u32[nm+1] | tmp | flg, lab, mark u8[n]
    Carve W;
    const size_t o_pos = W.add<uint64_t>(n), o_nxa = W.add<uint32_t>(n), o_nxb = W.add<uint32_t>(n), o_minc = W.add<uint32_t>(n);
    const size_t o_lbl = W.add<uint32_t>(n), o_rank = W.add<uint32_t>(n), o_item = W.add<uint32_t>(n), o_midx = W.add<uint32_t>((size_t)nm + 1);
    const size_t o_tmp = W.add<uint32_t>(sf::any_scan_tmp_words(n)), o_flg = W.add<uint8_t>(n), o_lab = W.add<uint8_t>(n), o_mark = W.add<uint8_t>(n);
    if ((rc = ctx->d_any.grow(ctx, W.bytes(), "walk nodes"))) return rc;
    uint8_t* b = ctx->d_any;
    uint64_t* pos = Carve::at<uint64_t>(b, o_pos);
    auto u32 = [b](size_t off) { return Carve::at<uint32_t>(b, off); };
    if (prof) SF_HIP(hipEventRecord(ctx->ev_any[2], s), "event");
    SF_HIP(sf::launch_any_nodes(t_items, t_waves, heads, nwaves, cn, cm, pos, b + o_flg, u32(o_minc), u32(o_midx), u32(o_item), s),
           "launch k_any_scan");
    if (prof) SF_HIP(hipEventRecord(ctx->ev_any[3], s), "event");
    SF_HIP(sf::launch_any_walk(t_items, heads, range, u32(o_item), pos, b + o_flg, u32(o_minc), u32(o_midx), n, largest, u32(o_nxa),
                               u32(o_nxb), b + o_lab, b + o_mark, u32(o_lbl), u32(o_rank), u32(o_tmp), tot + 2, d_index, ok, s),
           "launch k_any_walk");
    if (prof) SF_HIP(hipEventRecord(ctx->ev_any[4], s), "event");
  }
  SF_HIP(hipMemcpyAsync(okv.data(), ok, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "D2H walk");
  if (!trailer && container) SF_HIP(hipMemcpyAsync(rows.data(), ctx->tab.d, b_rows, hipMemcpyDeviceToHost, s), "D2H wrapper rows");
  if ((rc = mark_call_end(ctx, s)) != SFH_OK) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  if (prof && nwaves) {
    float a = 0, c = 0, w = 0;
    SF_HIP(hipEventElapsedTime(&a, ctx->ev_any[0], ctx->ev_any[1]), "elapsed");
    SF_HIP(hipEventElapsedTime(&c, ctx->ev_any[2], ctx->ev_any[3]), "elapsed");
    SF_HIP(hipEventElapsedTime(&w, ctx->ev_any[3], ctx->ev_any[4]), "elapsed");
    ctx->any_ms[0] = a + c;
    ctx->any_ms[1] = w;
  }
  for (size_t i = 0; i < count; ++i) {
    if (!R.st[i] && rows[i].wst) R.st[i] = rows[i].wst;  // container.hpp's answer for the wrapper
    if (!R.st[i] && !okv[i]) R.st[i] = SFH_ITEM_NOT_INDEXABLE;
    R.take[i] = R.st[i] == 0;
  }
  ctx->index_valid = false;
  ctx->bix_valid = false;
  return SFH_OK;
}

// The decoder on the flat recovered index, over the items the recovery kept (R.take): the batch decoder's tables and kernels,
// launch batch after launch batch of whole items (sf_any_plan.h) -- the token stage with the exact end rule and the
// reference's distance rule, the rows of dependent segments built on the device over the batch's segment table, the byte
// stage -- then the checksums and the fold.  The statuses land in R.st.  Synchronises s at the end.
// d_depends given (sfh_recover_index_device, a call of one item, which is always one launch batch): the token stage and the
// rows only -- the segments' depends flags are copied there, nothing is written through d_dsts (which may be null), and R.st
// stays as it is.
int any_batch_decode(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                     void* const* d_dsts, const uint64_t* d_index, hipStream_t s, AnyBatch& R, uint8_t* d_depends = nullptr) {
  const bool bytes_stage = d_depends == nullptr;
  sf::aplan::Plan P;
  try {
    sf::aplan::plan_batches(count, R.out_n.data(), R.take.data(), ctx->batch_chunks, P);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the launch batches", hipSuccess);
  }
  ctx->last_chunks = P.nseg;
  ctx->last_dtok_bytes = (size_t)P.widest * sf::kChunk * sizeof(uint32_t);
  ctx->ev_inf_valid = false;
  if (P.nseg == 0) return SFH_OK;
  const uint32_t nseg = P.nseg, nitems = P.nitems, nb = (uint32_t)P.batches.size(), wd = P.widest;
  int rc = ensure_seginfo(ctx, (size_t)nseg);
  if (!rc) rc = ensure_dtok(ctx, wd);
  if (!rc && container) rc = ensure_sums(ctx, nseg);
  if (!rc) rc = ensure_bstatus(ctx, (size_t)nitems + nb);
  // rows per batch u32[nb] | depends u8[wd] | starts, excl u32[wd] | tmp | rows InflateStrip[wd]
  Carve D;
  const size_t o_nrows = D.add<uint32_t>(nb), o_dep = D.add<uint8_t>(wd), o_st = D.add<uint32_t>(wd), o_ex = D.add<uint32_t>(wd);
  const size_t o_tmp = D.add<uint32_t>(sf::any_scan_tmp_words(wd)), o_rows = D.add<sf::InflateStrip>(wd);
  if (!rc) rc = ctx->d_anyseg.grow(ctx, D.bytes(), "segment rows");
  if (rc) return rc;
  // the tables, in one pinned block: segments | items | checksum chunks
  Carve L;
  const size_t o_segs = L.add<sf::InflateSeg>(nseg), o_items = L.add<sf::InflateItem>(nitems);
  const size_t o_sums = L.add<sf::BatchChunk>(container ? nseg : 0), bytes = L.bytes();
  if ((rc = ctx->tab.stage(ctx, bytes)) != SFH_OK) return rc;
  sf::InflateSeg* h_segs = Carve::at<sf::InflateSeg>(ctx->tab.h, o_segs);
  sf::InflateItem* h_items = Carve::at<sf::InflateItem>(ctx->tab.h, o_items);
  sf::BatchChunk* h_sums = Carve::at<sf::BatchChunk>(ctx->tab.h, o_sums);
  uint32_t g = 0, j = 0;
  for (size_t i = 0; i < count; ++i) {
    if (!R.take[i]) continue;
    const uint64_t out_n = R.out_n[i], body_n = body_bytes(container, src_n[i]);
    const uint32_t n = sf::aplan::segments_of(out_n);
    const uint64_t* ix = d_index + R.ix0[i];
    h_items[j++] = sf::InflateItem{(const uint8_t*)d_srcs[i], src_n[i], out_n, nullptr, ix, g, n, 0, 0, 0, 0};
    for (uint32_t k = 0; k < n; ++k, ++g) {
      const uint64_t ob = (uint64_t)k * sf::kChunk;
      const uint32_t on = (uint32_t)std::min<uint64_t>(sf::kChunk, out_n - std::min(out_n, ob));
      const uint32_t hist = (k ? sf::kChunk : 0u) | (container ? sf::kSegWrapped : 0u) | (k + 1 < n ? sf::kSegExact : 0u);
      uint8_t* out = bytes_stage ? (uint8_t*)d_dsts[i] + ob : nullptr;
      h_segs[g] = sf::InflateSeg{(const uint8_t*)d_srcs[i], ix + k, nullptr, out, body_n, on, hist};
      if (container) h_sums[g] = sf::BatchChunk{out, on, 0u};
    }
  }
  sf::InflateSeg* t_segs = Carve::at<sf::InflateSeg>(ctx->tab.d, o_segs);
  sf::InflateItem* t_items = Carve::at<sf::InflateItem>(ctx->tab.d, o_items);
  sf::BatchChunk* t_sums = Carve::at<sf::BatchChunk>(ctx->tab.d, o_sums);
  uint8_t* sb = ctx->d_anyseg;
  uint32_t* d_nrows = Carve::at<uint32_t>(sb, o_nrows);
  sf::InflateStrip* strips = Carve::at<sf::InflateStrip>(sb, o_rows);
  const bool prof = ctx->profiling != 0;
  if ((rc = ctx->tab.upload(ctx, bytes, s)) != SFH_OK) return rc;
  if (prof && (rc = ensure_inflate_events(ctx, nb)) != SFH_OK) return rc;
  SF_HIP(sf::launch_inflate_head(t_items, nitems, container, t_segs, container ? t_sums : nullptr, s), "launch k_inflate_head");
  for (uint32_t bi = 0; bi < nb; ++bi) {
    const sf::aplan::Batch& b = P.batches[bi];
    sf::SegInfo* binfo = ctx->ws.seginfo + b.row0;
    Event* ev = prof ? &ctx->ev_inf[(size_t)bi * (SFH_INFLATE_NSTAGES + 1)] : nullptr;
    if (ev) SF_HIP(hipEventRecord(ev[0], s), "event");
    SF_HIP(sf::launch_inflate_tokens_exact(t_segs + b.row0, b.nseg, ctx->ws.tokens, binfo, !ctx->inflate_serial, s),
           "launch k_inflate_tokens");
    SF_HIP(sf::launch_any_rows(t_segs + b.row0, binfo, ctx->ws.tokens, b.nseg, sb + o_dep, Carve::at<uint32_t>(sb, o_st),
                               Carve::at<uint32_t>(sb, o_ex), Carve::at<uint32_t>(sb, o_tmp), d_nrows + bi, strips, s), "launch k_any_rows");
    if (ev) SF_HIP(hipEventRecord(ev[1], s), "event");
    if (bytes_stage) SF_HIP(sf::launch_inflate_bytes(t_segs + b.row0, strips, b.nseg, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes");
    if (ev) SF_HIP(hipEventRecord(ev[2], s), "event");
  }
  ctx->ev_inf_batches = nb;
  ctx->ev_inf_valid = prof;
  // statuses u32[nitems] (not without the byte stage) | rows per batch u32[nb]
  const size_t first = bytes_stage ? 0 : nitems;
  if (bytes_stage) {
    if (container) SF_HIP(sf::launch_checksum_batch(t_sums, nseg, container, ctx->ws.sums, s), "launch k_checksum");
    SF_HIP(sf::launch_inflate_fold(t_items, nitems, ctx->ws.seginfo, ctx->ws.sums, container, ctx->bstatus.d, nullptr, s),
           "launch k_inflate_fold");
  } else {
    SF_HIP(hipMemcpyAsync(d_depends, sb + o_dep, nseg, hipMemcpyDeviceToDevice, s), "copy depends");
  }
  SF_HIP(hipMemcpyAsync(ctx->bstatus.d + nitems, d_nrows, nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, s), "copy rows");
  SF_HIP(hipMemcpyAsync(ctx->bstatus.h + first, ctx->bstatus.d + first, ((size_t)nitems + nb - first) * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, s), "copy statuses");
  if ((rc = mark_call_end(ctx, s)) != SFH_OK) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  j = 0;
  for (size_t i = 0; i < count && bytes_stage; ++i)
    if (R.take[i]) R.st[i] = ctx->bstatus.h[j++];
  for (uint32_t bi = 0; bi < nb; ++bi) ctx->any_counts[1] += ctx->bstatus.h[nitems + bi];
  return SFH_OK;
}

// ---- streams without flush points (sfh_inflate_stream*, sfh_inflate_stream_batch*; sf_stream.hip) ----
// the containers these calls take, and no other: the decoders', and a file of gzip members
bool stream_container(uint32_t container) { return container <= SFH_GZIP || container == SFH_GZIP_MEMBERS; }

// Everything a batched call checks before it enqueues anything (`dev`: device buffers, the single call's alignment rules).
int check_stream_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                       void* const* dsts, const uint64_t* dst_cap, const uint64_t* dst_n_out, const uint32_t* status, bool dev) {
  if (!ctx || !stream_container(container)) return fail(ctx, SFH_E_INVALID_ARG, "argument (container)", hipSuccess);
  if (count == 0) return SFH_OK;
  if (!srcs || !src_n || !dst_n_out || !status || (dsts && !dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  const uint64_t S = ctx->stream_chunk;
  uint64_t nc = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((!srcs[i] && src_n[i]) || (dsts && !dsts[i] && dst_cap[i])) return fail(ctx, SFH_E_INVALID_ARG, "null item pointer", hipSuccess);
    if (dev && (((uintptr_t)srcs[i] & 3) || (dsts && ((uintptr_t)dsts[i] & 15))))
      return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
    if (dsts && dst_cap[i] > ((uint64_t)1 << 44)) return fail(ctx, SFH_E_INVALID_ARG, "dst_cap: at most 2^44", hipSuccess);
    nc += src_n[i] ? (src_n[i] + S - 1) / S : 1;  // (at least the body's nominal chunks)
  }
  if (nc > ((uint64_t)1 << 31) - 1)
    return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 nominal chunks in one call (SFH_STREAM_CHUNK)", hipSuccess);
  return dsts ? check_disjoint(ctx, dsts, dst_cap, count) : SFH_OK;
}

// The one driver: a single stream is a call of one item.  Arguments checked, count > 0.  Item i is decoded when dsts && dsts[i]
// (else it is a size query: steps A to C only); stage: into ctx->d_out at (*out_off)[i] instead (the host-buffer entry points).
// The wrappers (k_inflate_head), then A to C for every item at once -- the candidate filter, the count pass, the chain rounds
// with a follow launch until the last item's chain is complete, the scan of the counts -- then D to F (write pass, resolve) and
// the checksums in launch batches of whole items of at most batch_chunks * 32 KiB of output each.  Host synchronisations: the
// wrapper (not for raw items), the candidates, the count pass and each chain round, and per launch batch the statuses and the
// checksums.
int stream_batch_run(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                     void* const* dsts, const uint64_t* dst_cap, bool stage, std::vector<uint64_t>* out_off, uint64_t* dst_n_out,
                     uint32_t* status, hipStream_t s, const uint64_t* lead = nullptr) {
  // lead (raw items only; null: none): bytes of item i in front of its body -- a ZIP entry's data inside the aligned item around it
  // members: every item is a file of gzip members.  Its wrapper is its first member's header (wrap: the container whose head
  // and checksum kernels serve), its body reaches to its last byte, its records have side rows, and its trailers are checked
  // per member behind each launch batch ("Files of members")
  const bool members = container == SFH_GZIP_MEMBERS;
  const uint32_t wrap = members ? (uint32_t)SFH_GZIP : container;
  ctx->stm_members.clear();
  const auto call_end = [&]() -> int {
    const int rc = mark_call_end(ctx, s);
    ctx->stm_members_valid = !rc && members;
    return rc;
  };
  const bool prof = ctx->profiling != 0;
  for (float& m : ctx->stm_ms) m = 0;
  for (uint64_t& c : ctx->stm_counts) c = 0;
  ctx->last_dtok_bytes = 0;
  for (size_t i = 0; i < count; ++i) dst_n_out[i] = status[i] = 0;
  if (stage) {
    try {
      out_off->assign(count + 1, 0);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
    }
  }
  for (Event& e : ctx->ev_stm)
    if (!e) SF_HIP(hipEventCreate(&e.h), "event");
  auto lap = [&](int a, int b, int stage_ix) -> int {
    float ms = 0;
    SF_HIP(hipEventElapsedTime(&ms, ctx->ev_stm[a], ctx->ev_stm[b]), "elapsed");
    ctx->stm_ms[stage_ix] += ms;
    return SFH_OK;
  };
  const uint64_t S = ctx->stream_chunk, kBig = (uint64_t)1 << 44;
  const auto decodes = [&](size_t i) { return dsts && dsts[i]; };
  std::vector<sf::InflateItem> head;
  std::vector<uint64_t> body;
  std::vector<uint32_t> live;  // the items whose body is decoded, in call order: their rows in `items`
  std::vector<sf::StreamItem> items;
  try {
    head.resize(count);
    body.resize(2 * count);
    live.reserve(count);
    items.reserve(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the item rows", hipSuccess);
  }
  int rc = order_behind_last_call(ctx, s);
  if (rc) return rc;
  // the wrappers: k_inflate_head over every item, as any_wrapper reads one (a raw body is the whole item: no launch, no wait)
  Carve T;  // wrapper rows | bodies | item rows
  const size_t o_head = T.add<sf::InflateItem>(count), o_body = T.add<uint64_t>(2 * count), o_items = T.add<sf::StreamItem>(count);
  if ((rc = ctx->d_sbt.grow(ctx, T.bytes(), "stream item rows"))) return rc;
  sf::InflateItem* d_head = Carve::at<sf::InflateItem>(ctx->d_sbt, o_head);
  uint64_t* d_body = Carve::at<uint64_t>(ctx->d_sbt, o_body);
  sf::StreamItem* d_items = Carve::at<sf::StreamItem>(ctx->d_sbt, o_items);
  if (container != SFH_RAW) {
    for (size_t i = 0; i < count; ++i)
      head[i] = sf::InflateItem{(const uint8_t*)srcs[i], src_n[i], decodes(i) && !members ? dst_cap[i] : kBig, d_body + 2 * i,
                                nullptr, 0, 0, 0, 0, 0, 0};  // (members: the last trailer's ISIZE says nothing about the file)
    SF_HIP(hipMemcpyAsync(d_head, head.data(), sizeof(sf::InflateItem) * count, hipMemcpyHostToDevice, s), "H2D wrapper rows");
    SF_HIP(sf::launch_inflate_head(d_head, (uint32_t)count, wrap, nullptr, nullptr, s), "launch k_inflate_head");
    SF_HIP(hipMemcpyAsync(head.data(), d_head, sizeof(sf::InflateItem) * count, hipMemcpyDeviceToHost, s), "D2H wrapper rows");
    SF_HIP(hipMemcpyAsync(body.data(), d_body, 16 * count, hipMemcpyDeviceToHost, s), "D2H bodies");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
  }
  uint64_t nc64 = 0;
  for (size_t i = 0; i < count; ++i) {
    if (container == SFH_RAW) {
      if (src_n[i] == (lead ? lead[i] : 0)) {  // no header bits at all
        status[i] = sf::inflate::kInvalidBlockHeader;
        continue;
      }
      body[2 * i] = lead ? lead[i] : 0;
      body[2 * i + 1] = src_n[i];
    } else if (head[i].wst) {
      status[i] = head[i].wst;
      continue;
    }
    const uint64_t bn = (members ? src_n[i] : body[2 * i + 1]) - body[2 * i];
    sf::StreamItem it{};
    it.src = (const uint8_t*)srcs[i];
    it.src_n = src_n[i];
    it.b0 = body[2 * i];
    it.body_n = bn;
    it.c0 = (uint32_t)nc64;
    nc64 += bn ? (bn + S - 1) / S : 1;
    live.push_back((uint32_t)i);
    items.push_back(it);
  }
  const uint32_t nl = (uint32_t)live.size();
  if (nl == 0) return call_end();
  if (nc64 >= ((uint64_t)1 << 31)) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 nominal chunks (SFH_STREAM_CHUNK)", hipSuccess);
  const uint32_t nc = (uint32_t)nc64;
  // cand u64[nc] (then: the records' items u32[nc] | the follow list u32[nc]) | recs StreamChunk[nc] | list u32[nc] | members:
  // side StreamSide[nc]
  Carve C;
  const size_t o_cand = C.add<uint64_t>(nc), o_rec = C.add<sf::StreamChunk>(nc), o_list = C.add<uint32_t>(nc);
  const size_t o_side = C.add<sf::StreamSide>(members ? nc : 0);
  size_t stm_bytes = C.bytes();
  if ((rc = ctx->d_stm.grow(ctx, stm_bytes, "stream chunk records"))) return rc;
  sf::StreamSide* d_side = members ? Carve::at<sf::StreamSide>(ctx->d_stm, o_side) : nullptr;
  sf::StreamMember* d_mem = nullptr;
  std::vector<sf::StreamSide> side;
  uint64_t* d_cand = Carve::at<uint64_t>(ctx->d_stm, o_cand);
  uint32_t* d_rec_item = Carve::at<uint32_t>(ctx->d_stm, o_cand);
  uint32_t* d_follow = d_rec_item + nc;
  sf::StreamChunk* d_rec = Carve::at<sf::StreamChunk>(ctx->d_stm, o_rec);
  uint32_t* d_list = Carve::at<uint32_t>(ctx->d_stm, o_list);
  std::vector<uint64_t> cand;
  std::vector<sf::StreamChunk> rec;
  std::vector<uint32_t> rec_item, chain(nl, 0);
  try {
    cand.resize(nc);
    rec.reserve(nc);
    rec_item.reserve(nc);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the chunk records", hipSuccess);
  }
  // A: candidates, every item's nominal chunks at once
  SF_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(sf::StreamItem) * nl, hipMemcpyHostToDevice, s), "H2D item rows");
  if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[0], s), "event");
  SF_HIP(sf::launch_stream_find(d_items, nl, nc, S, d_cand, s, members), "launch k_stream_find");
  if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[1], s), "event");
  SF_HIP(hipMemcpyAsync(cand.data(), d_cand, 8 * (size_t)nc, hipMemcpyDeviceToHost, s), "D2H candidates");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  for (uint32_t k = 0; k < nl; ++k) {
    sf::StreamItem& it = items[k];
    const uint32_t c1 = k + 1 < nl ? items[k + 1].c0 : nc;
    it.r0 = (uint32_t)rec.size();
    for (uint32_t c = it.c0; c < c1; ++c)
      if (cand[c] != sf::kNoCandidate && (rec.size() == it.r0 || cand[c] > rec.back().start)) {
        rec.push_back(sf::StreamChunk{cand[c], 0, 0, 0, 0, 0, 0});
        rec_item.push_back(k);
      }
    it.m = (uint32_t)rec.size() - it.r0;
    for (uint32_t i = it.r0; i < it.r0 + it.m; ++i) rec[i].limit = i + 1 < it.r0 + it.m ? rec[i + 1].start : ~0ull;
  }
  const uint32_t M = (uint32_t)rec.size();
  // B and C: the count pass over every record, then rounds of repairs until every item's chain reaches its end
  const size_t rec_bytes = sizeof(sf::StreamChunk) * (size_t)M;
  SF_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(sf::StreamItem) * nl, hipMemcpyHostToDevice, s), "H2D item rows");
  SF_HIP(hipMemcpyAsync(d_rec_item, rec_item.data(), 4 * (size_t)M, hipMemcpyHostToDevice, s), "H2D record items");
  SF_HIP(hipMemcpyAsync(d_rec, rec.data(), rec_bytes, hipMemcpyHostToDevice, s), "H2D chunk records");
  SF_HIP(sf::launch_stream_decode(false, d_items, d_rec_item, d_rec, nullptr, M, false, nullptr, s, d_side), "launch k_stream_decode");
  SF_HIP(hipMemcpyAsync(rec.data(), d_rec, rec_bytes, hipMemcpyDeviceToHost, s), "D2H chunk records");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  std::vector<char> done(nl, 0);
  std::vector<uint32_t> redo, follow;
  uint32_t rounds = 0;
  for (;;) {
    redo.clear();
    follow.clear();
    for (uint32_t k = 0; k < nl; ++k) {
      if (done[k]) continue;
      const size_t before = redo.size();
      sf::stream_chain_round(rec.data(), items[k].r0, items[k].m, redo, &chain[k]);
      if (redo.size() == before) {
        done[k] = 1;
      } else {
        follow.push_back(redo[before]);  // behind the item's confirmed chain: it goes on through the broken links after it
      }
    }
    if (redo.empty()) break;
    ++rounds;
    SF_HIP(hipMemcpyAsync(d_rec, rec.data(), rec_bytes, hipMemcpyHostToDevice, s), "H2D chunk records");
    SF_HIP(hipMemcpyAsync(d_list, redo.data(), 4 * redo.size(), hipMemcpyHostToDevice, s), "H2D repair list");
    SF_HIP(hipMemcpyAsync(d_follow, follow.data(), 4 * follow.size(), hipMemcpyHostToDevice, s), "H2D follow list");
    SF_HIP(sf::launch_stream_decode(false, d_items, d_rec_item, d_rec, d_list, (uint32_t)redo.size(), false, nullptr, s, d_side),
           "launch k_stream_decode");
    SF_HIP(sf::launch_stream_decode(false, d_items, d_rec_item, d_rec, d_follow, (uint32_t)follow.size(), true, nullptr, s, d_side),
           "launch k_stream_decode");
    SF_HIP(hipMemcpyAsync(rec.data(), d_rec, rec_bytes, hipMemcpyDeviceToHost, s), "D2H chunk records");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
  }
  if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[2], s), "event");
  if (members) {  // the side rows as the last decode of each record left them
    try {
      side.resize(M);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory for the side rows", hipSuccess);
    }
    SF_HIP(hipMemcpyAsync(side.data(), d_side, sizeof(sf::StreamSide) * (size_t)M, hipMemcpyDeviceToHost, s), "D2H side rows");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
  }
  std::vector<uint64_t> total(nl, 0), mem0(nl + 1, 0);  // mem0: an item's first member row (decoded items only)
  uint64_t longest = 0, confirmed = 0;
  for (uint32_t k = 0; k < nl; ++k) {
    sf::StreamItem& it = items[k];
    for (uint32_t i = it.r0; i < it.r0 + chain[k]; ++i) {
      rec[i].base = total[k];
      total[k] += rec[i].out;
      longest = std::max(longest, rec[i].out);
    }
    it.chain = chain[k];
    it.G = sf::stream_group(chain[k]);
    confirmed += chain[k];
    dst_n_out[live[k]] = total[k];
    if (!decodes(live[k])) status[live[k]] = rec[it.r0 + chain[k] - 1].status;
    mem0[k + 1] = members && decodes(live[k]) ? sf::stream_member_scan(rec.data(), side.data(), it.r0, chain[k], mem0[k]) : mem0[k];
  }
  if (mem0[nl] > ((uint64_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 members in one call", hipSuccess);
  if (mem0[nl]) {
    if ((rc = ctx->d_smem.grow(ctx, sizeof(sf::StreamMember) * mem0[nl], "member rows"))) return rc;
    d_mem = Carve::at<sf::StreamMember>(ctx->d_smem, 0);
    stm_bytes += sizeof(sf::StreamMember) * mem0[nl];
  }
  ctx->stm_counts[0] = nc;
  ctx->stm_counts[1] = M;
  ctx->stm_counts[2] = confirmed;
  ctx->stm_counts[3] = rounds;
  ctx->stm_counts[4] = longest;
  ctx->stm_counts[5] = stm_bytes;
  ctx->last_dtok_bytes = stm_bytes;
  if (prof) {
    SF_HIP(hipEventSynchronize(ctx->ev_stm[2]), "event sync");
    if ((rc = lap(0, 1, 0)) || (rc = lap(1, 2, 1))) return rc;
  }
  // D to F in launch batches of whole items: each item's plane and windows at its place in its batch's
  const uint64_t budget = (uint64_t)ctx->batch_chunks * sf::kChunk;
  std::vector<uint32_t> dec;  // the decoded items' rows, and where each launch batch starts among them
  std::vector<size_t> lb;
  if (stage) {
    uint64_t o = 0;
    for (size_t i = 0, k = 0; i < count; ++i) {
      (*out_off)[i] = o;
      if (k < nl && live[k] == i) {
        if (decodes(i)) o += al16(std::min(total[k], container == SFH_GZIP ? (uint64_t)head[i].isize : dst_cap[i]));  // (as it.cap)
        ++k;
      }
    }
    (*out_off)[count] = o;
    if ((rc = ctx->d_out.grow(ctx, std::max<uint64_t>(16, o), "output staging"))) return rc;
  }
  uint64_t cur = 0, peak = 0;
  for (uint32_t k = 0; k < nl; ++k) {
    const size_t i = live[k];
    if (!decodes(i)) continue;
    if (dec.empty() || (cur && cur + total[k] > budget)) {
      lb.push_back(dec.size());
      cur = 0;
    }
    dec.push_back(k);
    cur += total[k];
  }
  lb.push_back(dec.size());
  std::vector<uint64_t> plane_n(lb.size(), 0), wins_n(lb.size(), 0);
  for (size_t b = 0; b + 1 < lb.size(); ++b)
    for (size_t q = lb[b]; q < lb[b + 1]; ++q) {
      sf::StreamItem& it = items[dec[q]];
      const size_t i = live[dec[q]];
      it.plane = plane_n[b];
      it.win = wins_n[b];
      it.cap = container == SFH_GZIP ? (uint64_t)head[i].isize : dst_cap[i];  // (container.hpp: a gzip body into dst.first(ISIZE))
      it.dst = stage ? ctx->d_out + (*out_off)[i] : (uint8_t*)dsts[i];
      plane_n[b] += al16(total[dec[q]]);  // (entries; 16-entry aligned)
      wins_n[b] += (uint64_t)((it.chain + it.G - 1) / it.G - 1) * 32768;
    }
  if (!dec.empty()) {
    SF_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(sf::StreamItem) * nl, hipMemcpyHostToDevice, s), "H2D item rows");
    SF_HIP(hipMemcpyAsync(d_rec, rec.data(), rec_bytes, hipMemcpyHostToDevice, s), "H2D chunk records");
    if (members) SF_HIP(hipMemcpyAsync(d_side, side.data(), sizeof(sf::StreamSide) * (size_t)M, hipMemcpyHostToDevice, s), "H2D side rows");
  }
  std::vector<sf::StreamMember> mrow;  // members: a launch batch's member rows, and per fold row its member in them
  std::vector<uint32_t> fold_mem, whole;  // whole: the batch's items whose bodies decoded
  std::vector<uint32_t> wlist, link, bst;
  std::vector<sf::StreamGroup> compose, resolve;
  std::vector<sf::BatchChunk> sums;
  std::vector<sf::InflateItem> fold;
  std::vector<uint32_t> fold_item;
  for (size_t b = 0; b + 1 < lb.size(); ++b) {
    const size_t q0 = lb[b], q1 = lb[b + 1];
    const size_t wins_bytes = 2 * wins_n[b], plane_bytes = std::max<size_t>(16, 2 * plane_n[b]);
    peak = std::max<uint64_t>(peak, plane_bytes + wins_bytes);
    if ((rc = ctx->d_plane.grow(ctx, plane_bytes / 2, "symbol plane"))) return rc;
    if (wins_bytes && (rc = ctx->d_wins.grow(ctx, wins_bytes / 2, "stream windows"))) return rc;
    // D: the confirmed records of the batch's items
    wlist.clear();
    for (size_t q = q0; q < q1; ++q) {
      const sf::StreamItem& it = items[dec[q]];
      for (uint32_t i = it.r0; i < it.r0 + it.chain; ++i) wlist.push_back(i);
    }
    const uint32_t ra = items[dec[q0]].r0, rb = items[dec[q1 - 1]].r0 + items[dec[q1 - 1]].m;
    if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[2], s), "event");
    SF_HIP(hipMemcpyAsync(d_list, wlist.data(), 4 * wlist.size(), hipMemcpyHostToDevice, s), "H2D write list");
    SF_HIP(sf::launch_stream_decode(true, d_items, d_rec_item, d_rec, d_list, (uint32_t)wlist.size(), false, ctx->d_plane, s, d_side,
                                    d_mem),
           "launch k_stream_decode");
    if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[3], s), "event");
    SF_HIP(hipMemcpyAsync(rec.data() + ra, d_rec + ra, sizeof(sf::StreamChunk) * (size_t)(rb - ra), hipMemcpyDeviceToHost, s),
           "D2H chunk records");
    const uint64_t ma = mem0[dec[q0]], mb = mem0[dec[q1 - 1] + 1];  // the batch's member rows (an item not decoded has none)
    if (members && mb > ma) {
      try {
        mrow.resize(mb - ma);
      } catch (...) {
        return fail(ctx, SFH_E_NOMEM, "host memory for the member rows", hipSuccess);
      }
      SF_HIP(hipMemcpyAsync(mrow.data(), d_mem + ma, sizeof(sf::StreamMember) * (mb - ma), hipMemcpyDeviceToHost, s), "D2H member rows");
    }
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    if (prof && (rc = lap(2, 3, 2))) return rc;
    // the statuses; E / F for the items that decoded, then their checksums
    compose.clear();
    resolve.clear();
    link.clear();
    sums.clear();
    fold.clear();
    fold_item.clear();
    fold_mem.clear();
    whole.clear();
    for (size_t q = q0; q < q1; ++q) {
      const uint32_t k = dec[q];
      const sf::StreamItem& it = items[k];
      const size_t i = live[k];
      uint32_t st = 0;
      for (uint32_t r = it.r0; r < it.r0 + it.chain && !st; ++r) st = rec[r].status;
      if (!st && container == SFH_GZIP && total[k] != head[i].isize) st = sf::inflate::kError;
      status[i] = st;
      if (st) continue;
      const uint32_t ng = (it.chain + it.G - 1) / it.G;
      for (uint32_t g = 0; g < ng; ++g) {
        if (g + 1 < ng) compose.push_back(sf::StreamGroup{k, g});
        resolve.push_back(sf::StreamGroup{k, g});
      }
      if (ng > 1) link.push_back(k);
      if (members) {
        whole.push_back(k);
        // one fold row per member, its checksum rows of at most 32 KiB from wherever its output starts; ISIZE from the row
        uint64_t o = 0;
        for (uint64_t r = mem0[k]; r < mem0[k + 1]; ++r) {
          sf::StreamMember& m = mrow[r - ma];
          const uint64_t n = m.out_end - o;
          m.item = (uint32_t)i;
          m.status = m.isize != (uint32_t)n;
          if (m.status) status[i] = sf::inflate::kError;
          fold.push_back(sf::InflateItem{it.src, it.src_n, n, nullptr, nullptr, (uint32_t)sums.size(), 0, 0, m.crc32,
                                         (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFu), 0});
          fold_item.push_back((uint32_t)i);
          fold_mem.push_back((uint32_t)(r - ma));
          for (uint64_t ob = 0; ob < n || ob == 0; ob += sf::kChunk)
            sums.push_back(sf::BatchChunk{n ? it.dst + o + ob : (const uint8_t*)ctx->d_plane.p, (uint32_t)std::min<uint64_t>(sf::kChunk, n - ob), 0u});
          o = m.out_end;
        }
      } else if (container) {
        const uint32_t nch = chunks_of((size_t)total[k]);
        fold.push_back(sf::InflateItem{it.src, it.src_n, total[k], nullptr, nullptr, (uint32_t)sums.size(), 0, 0, head[i].want,
                                       (uint32_t)total[k], 0});
        fold_item.push_back((uint32_t)i);
        for (uint32_t c = 0; c < nch; ++c) {
          const uint64_t ob = (uint64_t)c * sf::kChunk;
          // (an empty output: one empty row, at a real address)
          sums.push_back(sf::BatchChunk{total[k] ? it.dst + ob : (const uint8_t*)ctx->d_plane.p, (uint32_t)std::min<uint64_t>(sf::kChunk, total[k] - ob), 0u});
        }
      }
    }
    if (resolve.empty()) continue;
    // compose | resolve | link | checksum rows | fold rows | fold statuses
    Carve G;
    const size_t o_comp = G.add<sf::StreamGroup>(compose.size()), o_res = G.add<sf::StreamGroup>(resolve.size());
    const size_t o_link = G.add<uint32_t>(link.size()), o_sums = G.add<sf::BatchChunk>(sums.size());
    const size_t o_fold = G.add<sf::InflateItem>(fold.size()), o_fst = G.add<uint32_t>(fold.size());
    if ((rc = ctx->d_sbr.grow(ctx, G.bytes(), "stream group rows"))) return rc;
    uint8_t* R = ctx->d_sbr;
    SF_HIP(hipMemcpyAsync(R + o_comp, compose.data(), 8 * compose.size(), hipMemcpyHostToDevice, s), "H2D group rows");
    SF_HIP(hipMemcpyAsync(R + o_res, resolve.data(), 8 * resolve.size(), hipMemcpyHostToDevice, s), "H2D group rows");
    if (!link.empty()) SF_HIP(hipMemcpyAsync(R + o_link, link.data(), 4 * link.size(), hipMemcpyHostToDevice, s), "H2D link rows");
    SF_HIP(sf::launch_stream_resolve(ctx->d_plane, d_rec, d_items, Carve::at<const sf::StreamGroup>(R, o_comp), (uint32_t)compose.size(),
                                     Carve::at<const uint32_t>(R, o_link), (uint32_t)link.size(), Carve::at<const sf::StreamGroup>(R, o_res),
                                     (uint32_t)resolve.size(), ctx->d_wins, s), "launch k_stream_resolve");
    if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[4], s), "event");
    if (!fold.empty()) {
      if ((rc = ensure_sums(ctx, (uint32_t)sums.size()))) return rc;
      SF_HIP(hipMemcpyAsync(R + o_sums, sums.data(), sizeof(sf::BatchChunk) * sums.size(), hipMemcpyHostToDevice, s), "H2D checksum rows");
      SF_HIP(hipMemcpyAsync(R + o_fold, fold.data(), sizeof(sf::InflateItem) * fold.size(), hipMemcpyHostToDevice, s), "H2D fold rows");
      if (members)
        SF_HIP(sf::launch_checksum_batch_any(Carve::at<const sf::BatchChunk>(R, o_sums), (uint32_t)sums.size(), ctx->ws.sums, s),
               "launch k_checksum_batch");
      else
        SF_HIP(sf::launch_checksum_batch(Carve::at<const sf::BatchChunk>(R, o_sums), (uint32_t)sums.size(), container, ctx->ws.sums, s),
               "launch k_checksum_batch");
      SF_HIP(sf::launch_inflate_fold(Carve::at<const sf::InflateItem>(R, o_fold), (uint32_t)fold.size(), nullptr, ctx->ws.sums, wrap,
                                     Carve::at<uint32_t>(R, o_fst), nullptr, s), "launch k_inflate_fold");
      bst.resize(fold.size());
      SF_HIP(hipMemcpyAsync(bst.data(), R + o_fst, 4 * fold.size(), hipMemcpyDeviceToHost, s), "D2H checksums");
    }
    if (prof) SF_HIP(hipEventRecord(ctx->ev_stm[5], s), "event");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    for (size_t f = 0; f < fold.size(); ++f) {
      if (!members) {
        status[fold_item[f]] = bst[f];
      } else if (bst[f]) {  // (an item's status: its first member that fails either check, and both are Error)
        status[fold_item[f]] = bst[f];
        mrow[fold_mem[f]].status = 1;
      }
    }
    if (members) {  // the table: the rows of the items whose bodies decoded, in call order
      try {
        for (const uint32_t k : whole)
          ctx->stm_members.insert(ctx->stm_members.end(), mrow.begin() + (mem0[k] - ma), mrow.begin() + (mem0[k + 1] - ma));
      } catch (...) {
        return fail(ctx, SFH_E_NOMEM, "host memory for the member table", hipSuccess);
      }
    }
    if (prof && ((rc = lap(3, 4, 3)) || (rc = lap(4, 5, 4)))) return rc;
  }
  ctx->stm_counts[5] = stm_bytes + peak;
  ctx->last_dtok_bytes = ctx->stm_counts[5];
  return call_end();
}

// A single stream: the driver with count == 1 (dst null: the size query; stage: dst is a host buffer, the bytes land at
// ctx->d_out).  The single calls' own argument checks stand in for check_stream_batch.
int stream_one(sfh_ctx* ctx, const void* d_src, uint64_t src_n, uint32_t container, void* dst, uint64_t dst_cap, bool stage,
               uint64_t* dst_n_out, uint32_t* status, hipStream_t s) {
  std::vector<uint64_t> out_off;
  const int rc = stream_batch_run(ctx, 1, &d_src, &src_n, container, dst ? &dst : nullptr, &dst_cap, stage, &out_off, dst_n_out,
                                  status, s);
  if (!rc && *status) snprintf(ctx->err, sizeof ctx->err, "DecompressStatus %u", *status);
  return rc;
}

int check_any(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, uint64_t dst_n, bool dev) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if ((!src && src_n) || container > SFH_GZIP) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (dev && ((uintptr_t)src & 3)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4)", hipSuccess);
  if (dst_n == SFH_SIZE_FROM_TRAILER ? container != SFH_GZIP : dst_n > ((uint64_t)1 << 44))
    return fail(ctx, SFH_E_INVALID_ARG, "dst_n: at most 2^44, or SFH_SIZE_FROM_TRAILER with a gzip stream", hipSuccess);
  return SFH_OK;
}

// The single calls are the driver's calls of one item.  What check_any_batch refuses for a whole call -- a count of scan waves
// that does not fit the driver's 32 bits -- is refused here for the one stream.
int check_any_waves(sfh_ctx* ctx, size_t src_n) {
  if (((uint64_t)src_n + 8191) / 8192 > ((uint64_t)1 << 31) - 1)
    return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 scan waves (a stream above 2^44 bytes)", hipSuccess);
  return SFH_OK;
}

}  // namespace

// ---- one process per GPU: concatenation over RCCL (bound at run time: a host without RCCL still loads the library) ----
namespace {
struct Rccl {
  // the subset of rccl.h this file calls (ncclResult_t is an int, ncclComm_t an opaque pointer, ncclUint8 = 1, ncclUint64 = 5)
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommCount)(const void*, int*) = nullptr;
  int (*CommUserRank)(const void*, int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
  char why[160] = {0};
};
const Rccl& rccl() {
  static const Rccl r = [] {
    Rccl x;
    void* h = nullptr;
    // the copy that is in the process already wins (a torch process has loaded its own librccl.so): two RCCLs, like two
    // HIP runtimes, must not serve one communicator
    const char* env = getenv("SFH_RCCL_LIB");
    const char* names[] = {env, "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names)
      if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char* n : names)
      if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      snprintf(x.why, sizeof x.why, "librccl.so not found (%s)", dlerror());
      return x;
    }
    auto sym = [&](const char* s) { return dlsym(h, s); };
    x.AllGather = (decltype(x.AllGather))sym("ncclAllGather");
    x.Send = (decltype(x.Send))sym("ncclSend");
    x.Recv = (decltype(x.Recv))sym("ncclRecv");
    x.GroupStart = (decltype(x.GroupStart))sym("ncclGroupStart");
    x.GroupEnd = (decltype(x.GroupEnd))sym("ncclGroupEnd");
    x.CommCount = (decltype(x.CommCount))sym("ncclCommCount");
    x.CommUserRank = (decltype(x.CommUserRank))sym("ncclCommUserRank");
    x.GetErrorString = (decltype(x.GetErrorString))sym("ncclGetErrorString");
    x.ok = x.AllGather && x.Send && x.Recv && x.GroupStart && x.GroupEnd && x.CommCount && x.CommUserRank;
    if (!x.ok) snprintf(x.why, sizeof x.why, "librccl.so lacks an ncclAllGather / ncclSend / ncclRecv / ncclGroup* symbol");
    return x;
  }();
  return r;
}
int comm_fail(sfh_ctx* ctx, const char* what, int code) {
  const Rccl& R = rccl();
  if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, R.GetErrorString ? R.GetErrorString(code) : "RCCL error");
  return SFH_E_COMM;
}
constexpr int kNcclUint8 = 1, kNcclUint64 = 5;
}  // namespace


extern "C" {

void sfh_default_options(sfh_options* o) {
  memset(o, 0, sizeof *o);
  o->strategy = SFH_AUTO;
  o->final_stream = 1;
  o->lazy = 3;
}

int sfh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sfh_get_device_props(int device, sfh_device_props* out) {
  if (!out) return SFH_E_INVALID_ARG;
  memset(out, 0, sizeof *out);
  const int n = sfh_device_count();
  if (n <= 0 || device < 0 || device >= n) return SFH_E_NO_DEVICE;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) return SFH_E_HIP;
  snprintf(out->name, sizeof out->name, "%s", p.name);
  snprintf(out->arch, sizeof out->arch, "%s", p.gcnArchName);
  out->compute_units = (uint32_t)p.multiProcessorCount;
  out->lds_bytes_per_cu = (uint32_t)p.maxSharedMemoryPerMultiProcessor;
  out->l2_bytes = (uint32_t)p.l2CacheSize;
  out->memory_clock_khz = (uint32_t)p.memoryClockRate;
  out->memory_bus_bits = (uint32_t)p.memoryBusWidth;
  out->clock_khz = (uint32_t)p.clockRate;
  out->total_memory = (uint64_t)p.totalGlobalMem;
  return SFH_OK;
}

int sfh_create(sfh_ctx** out, int device) {
  if (!out) return SFH_E_INVALID_ARG;
  *out = nullptr;
  int n = sfh_device_count();
  if (n <= 0 || device < 0 || device >= n) return SFH_E_NO_DEVICE;
  sfh_ctx* ctx = new (std::nothrow) sfh_ctx();
  if (!ctx) return SFH_E_NOMEM;
  ctx->device = device;
  {
    const char* e = getenv("SFH_K1_STAMPS");
    ctx->k1_stamps = (e && e[0] == '1');
    const char* b = getenv("SFH_BATCH_CHUNKS");
    if (b && atoi(b) > 0) ctx->batch_chunks = std::min<uint32_t>((uint32_t)atoi(b), sf::kBatchChunks);
    const char* f = getenv("SFH_FORCE_ORDER_FAIL");
    ctx->force_order_fail = (f && f[0] == '1');
    const char* q = getenv("SFH_INFLATE_SERIAL");
    ctx->inflate_serial = (q && q[0] == '1');
    const char* sc = getenv("SFH_STREAM_CHUNK");
    if (sc && atoll(sc) > 0) ctx->stream_chunk = (uint64_t)atoll(sc);
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&ctx->stream.h) != hipSuccess || ctx->d_total.grow(ctx, 1, "result slot") ||
      ctx->h_total.grow(ctx, 1, "result slot") || ctx->d_value.grow(ctx, 2, "result slot") || sf::init_kernels() != hipSuccess ||
      sf::init_inflate_kernels() != hipSuccess) {
    sfh_destroy(ctx);
    return SFH_E_HIP;
  }
  if (hipEventCreateWithFlags(&ctx->ev_done.h, hipEventDisableTiming) != hipSuccess) {
    sfh_destroy(ctx);
    return SFH_E_HIP;
  }
  for (int op = 0; op < 2; ++op) {  // the LDS ordering the chain and recent efforts rest on: settled here, once (see ensure_order)
    uint64_t bad = 0, checked = 0;
    if (check_order(ctx, op, &bad, &checked, 64, 4) == SFH_OK)
      ctx->order_ok[op] = (bad == 0 && checked != 0 && !ctx->force_order_fail) ? 1 : -1;
    ctx->err[0] = 0;  // (a check that could not run is run again by the first call that needs it, which then reports)
  }
  *out = ctx;
  return SFH_OK;
}

void sfh_destroy(sfh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;  // every member frees what it holds (sf_scratch.h), the context's stream last
}

const char* sfh_last_error(const sfh_ctx* ctx) { return ctx ? ctx->err : "null ctx"; }

int sfh_lds_order_check(sfh_ctx* ctx, uint32_t op, uint32_t blocks, uint32_t iters, uint64_t* mismatches, uint64_t* checked) {
  // (the kernel counts mismatches and checked positions with 32-bit atomics: blocks * iters * 1024 positions * 5 densities must fit,
  // and a launch at the bound still ends within seconds)
  if (!ctx || op > 1 || !blocks || blocks > 4096 || !iters || iters > 128 || !mismatches || !checked)
    return fail(ctx, SFH_E_INVALID_ARG, "argument (blocks 1..4096, iters 1..128)", hipSuccess);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  return check_order(ctx, (int)op, mismatches, checked, blocks, iters);
}


size_t sfh_compress_bound(size_t n, uint32_t block_bytes) {
  // per 32 KiB DEFLATE block: fixed-Huffman worst case (9 bits per literal) + headers + alignment block.  A strip is a
  // whole number of such blocks whatever block_bytes is, so a VALID block_bytes does not change the bound; one that
  // sfh_compress would reject (not a multiple of 32 KiB, above 16 MiB) gives 0: no buffer size makes that call succeed
  if (block_bytes && (block_bytes % sf::kChunk || block_bytes > sf::kMaxStrip)) return 0;
  const size_t nchunks = n ? (n + sf::kChunk - 1) / sf::kChunk : 1;
  return nchunks * (size_t)(sf::kChunk + sf::kChunk / 8 + 640);
}

size_t sfh_dz_header_bytes(size_t n) { return (size_t)sf::dz::header_bytes(n); }

size_t sfh_compress_bound_container(size_t n, uint32_t block_bytes, uint32_t container) {
  if (container > SFH_DICTZIP) return 0;
  if (container != SFH_DICTZIP) return sfh_compress_bound(n, block_bytes);
  if ((block_bytes && block_bytes != sf::kChunk) || n > sf::dz::kMaxInput) return 0;
  // (sfh_compress_bound covers the gzip header's 10 bytes: what comes on top is the extra field)
  return sfh_compress_bound(n, sf::kChunk) + (size_t)sf::dz::header_bytes(n) - 10;
}

int sfh_compress_device_async(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap,
                              uint64_t* d_out_n, const sfh_options* opt, void* stream) {
  if (!ctx) return SFH_E_INVALID_ARG;
  return enqueue(ctx, d_src, n, d_dst, cap, d_out_n, opt, stream ? (hipStream_t)stream : ctx->stream);
}

int sfh_compress_device(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap,
                        size_t* out_n, const sfh_options* opt, void* stream) {
  if (!ctx || !out_n) return SFH_E_INVALID_ARG;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  int rc = enqueue(ctx, d_src, n, d_dst, cap, ctx->d_total, opt, s);
  if (rc) return rc;
  SF_HIP(hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy size");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *out_n = (size_t)*ctx->h_total;
  return SFH_OK;
}

namespace {
// sfh_compress and sfh_compress_bgzf: host buffers, the batch loop moving the data as well
int compress_host(sfh_ctx* ctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n, const sfh_options* opt, bool bgzf) {
  if (!ctx || (!src && n) || !dst || !out_n) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  // (SFH_DICTZIP: the larger header needs the larger bound -- of the staging, and of the caller's buffer as well)
  const bool dictzip = !bgzf && opt && opt->container == SFH_DICTZIP;
  const size_t bound = bgzf ? sfh_bgzf_bound(n) : dictzip ? sfh_compress_bound_container(n, opt->block_bytes, SFH_DICTZIP) : sfh_compress_bound(n, 0);
  if (bgzf && (check_opt(opt) || (opt && (opt->container != SFH_RAW || opt->final_stream != 1 || (opt->block_bytes && opt->block_bytes != sf::kChunk)))))
    return fail(ctx, SFH_E_INVALID_ARG, "BGZF: container SFH_RAW, final_stream 1, block_bytes 0 or 32768", hipSuccess);
  if (bgzf && cap < bound) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_bgzf_bound(n)", hipSuccess);
  if (dictzip && !bound) return fail(ctx, SFH_E_INVALID_ARG, "SFH_DICTZIP: block_bytes 0 or 32768, n <= SFH_DZ_MAX_CHUNKS * 32768", hipSuccess);
  if (dictzip && check_opt(opt, true)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (dictzip && cap < bound) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_compress_bound_container(n)", hipSuccess);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = ctx->d_in.grow(ctx, n ? n : 16, "input staging");
  if (!rc) rc = ctx->d_out.grow(ctx, bound, "output staging");
  if (rc) return rc;
  if (!ctx->s_in) {  // the copy streams, their events and the pinned size slots: on first use
    SF_HIP(hipStreamCreateWithFlags(&ctx->s_in.h, hipStreamNonBlocking), "stream");
    SF_HIP(hipStreamCreateWithFlags(&ctx->s_out.h, hipStreamNonBlocking), "stream");
    for (int k = 0; k < sfh_ctx::kPipe; ++k) {
      SF_HIP(hipEventCreateWithFlags(&ctx->ev_in[k].h, hipEventDisableTiming), "event");
      SF_HIP(hipEventCreateWithFlags(&ctx->ev_batch[k].h, hipEventDisableTiming), "event");
    }
    if (ctx->h_tot.grow(ctx, sfh_ctx::kPipe, "pinned slots")) return SFH_E_HIP;  // (this call's code for it, as before)
  }
  hipStream_t s = ctx->stream;
  // the staging buffers may still be read by copies of the previous call: they were all waited for below
  HostPipe pipe{(const uint8_t*)src, (uint8_t*)dst, cap};
  rc = enqueue(ctx, ctx->d_in, n, ctx->d_out, bound, ctx->d_total, opt, s, &pipe, bgzf);
  if (rc) {
    (void)hipStreamSynchronize(ctx->s_in);
    (void)hipStreamSynchronize(s);
    (void)hipStreamSynchronize(ctx->s_out);
    return rc;
  }
  uint64_t total = 0;
  SF_HIP(hipMemcpyAsync(&total, ctx->d_total, sizeof total, hipMemcpyDeviceToHost, s), "copy size");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  if (pipe.overflow || total > cap) {
    (void)hipStreamSynchronize(ctx->s_out);
    return fail(ctx, SFH_E_DST_TOO_SMALL, "dst capacity below stream size", hipSuccess);
  }
  // a wrapped stream: the header in front and the trailer behind the raw bytes came last (k_wrap)
  const sfh_options* o = opt;
  const size_t hdr = dictzip ? sf::dz::header_bytes(n) : (!bgzf && o && o->container) ? sf::wrapper_header_bytes(o->container) : 0;
  if (hdr) SF_HIP(hipMemcpyAsync(dst, ctx->d_out, hdr, hipMemcpyDeviceToHost, ctx->s_out), "D2H header");
  if (total > pipe.copied)
    SF_HIP(hipMemcpyAsync((uint8_t*)dst + pipe.copied, ctx->d_out + pipe.copied, total - pipe.copied, hipMemcpyDeviceToHost, ctx->s_out), "D2H trailer");
  SF_HIP(hipStreamSynchronize(ctx->s_out), "stream sync");
  *out_n = (size_t)total;
  return SFH_OK;
}
}  // namespace

int sfh_compress(sfh_ctx* ctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n,
                 const sfh_options* opt) {
  return compress_host(ctx, src, n, dst, cap, out_n, opt, false);
}

// ---- BGZF, the writer ----
size_t sfh_bgzf_bound(size_t n) { return (size_t)sf::bgzf::bound(n); }

int sfh_compress_bgzf_device_async(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap, uint64_t* d_out_n,
                                   const sfh_options* opt, void* stream) {
  if (!ctx) return SFH_E_INVALID_ARG;
  return enqueue(ctx, d_src, n, d_dst, cap, d_out_n, opt, stream ? (hipStream_t)stream : ctx->stream, nullptr, true);
}

int sfh_compress_bgzf_device(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap, size_t* out_n,
                             const sfh_options* opt, void* stream) {
  if (!ctx || !out_n) return SFH_E_INVALID_ARG;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  int rc = enqueue(ctx, d_src, n, d_dst, cap, ctx->d_total, opt, s, nullptr, true);
  if (rc) return rc;
  SF_HIP(hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy size");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *out_n = (size_t)*ctx->h_total;
  return SFH_OK;
}

int sfh_compress_bgzf(sfh_ctx* ctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n, const sfh_options* opt) {
  return compress_host(ctx, src, n, dst, cap, out_n, opt, true);
}

int sfh_compress_batch_device_async(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                    void* const* d_dsts, const uint64_t* dst_cap, uint64_t* d_out_n,
                                    const sfh_options* opt, void* stream) {
  int rc = check_batch(ctx, count, d_srcs, src_n, d_dsts, dst_cap, d_out_n, opt, true);
  if (rc || count == 0) return rc;
  return enqueue_batch(ctx, count, d_srcs, src_n, d_dsts, d_out_n, opt, stream ? (hipStream_t)stream : ctx->stream);
}

int sfh_compress_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, void* const* dsts,
                       const uint64_t* dst_cap, uint64_t* out_n, const sfh_options* opt) {
  int rc = check_batch(ctx, count, srcs, src_n, dsts, dst_cap, out_n, opt, false);
  if (rc || count == 0) return rc;
  std::vector<uint64_t> slot;  // an item's output slot: its bound
  try {
    slot.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t i = 0; i < count; ++i) slot[i] = sfh_compress_bound((size_t)src_n[i], 0);
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, slot.data()))) return rc;
  if ((rc = ctx->bn.grow(ctx, count, "batch sizes"))) return rc;
  if ((rc = enqueue_batch(ctx, count, B.d_srcs.data(), src_n, B.d_dsts.data(), ctx->bn.d, opt, s)) != SFH_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  SF_HIP(hipMemcpyAsync(ctx->bn.h, ctx->bn.d, count * sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy sizes");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  for (size_t i = 0; i < count; ++i) out_n[i] = ctx->bn.h[i];
  return staged_down(ctx, B, count, dsts, out_n, nullptr);  // each item's stream
}

int sfh_batch_index_size(const sfh_ctx* ctx, size_t* items, size_t* entries) {
  if (!ctx || !items || !entries || !ctx->bix_valid) return SFH_E_INVALID_ARG;
  *items = ctx->bix_items;
  *entries = ctx->bix_entries;
  return SFH_OK;
}

int sfh_copy_batch_index(sfh_ctx* ctx, uint64_t* index, uint32_t* subindex, uint32_t* block_bytes, int dst_on_device, void* stream) {
  if (!ctx || !ctx->bix_valid) return fail(ctx, SFH_E_INVALID_ARG, "batch index: the last call on this context was no compress batch", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  if (int rc = order_behind_last_call(ctx, s)) return rc;  // written by the batch call's kernels, maybe on another stream
  const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t segs = ctx->bix_entries - ctx->bix_items;
  if (index) SF_HIP(hipMemcpyAsync(index, ctx->d_bix, ctx->bix_entries * sizeof(uint64_t), kind, s), "copy batch index");
  if (subindex) SF_HIP(hipMemcpyAsync(subindex, ctx->ws.subidx, segs * SFH_SUBINDEX_WORDS * sizeof(uint32_t), kind, s), "copy batch sub-index");
  if (block_bytes && dst_on_device)
    SF_HIP(hipMemcpyAsync(block_bytes, ctx->bix_block_bytes.data(), ctx->bix_items * sizeof(uint32_t), hipMemcpyHostToDevice, s),
           "copy block_bytes");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  if (block_bytes && !dst_on_device) memcpy(block_bytes, ctx->bix_block_bytes.data(), ctx->bix_items * sizeof(uint32_t));
  return SFH_OK;
}

int sfh_decompress_batch_device_async(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                      const uint64_t* d_index, const uint32_t* d_subindex, void* const* d_dsts,
                                      const uint64_t* dst_n, const uint32_t* block_bytes, uint32_t container,
                                      uint32_t* d_status, void* stream) {
  int rc = check_inflate_batch(ctx, count, d_srcs, src_n, d_index, d_subindex, d_dsts, dst_n, block_bytes, container, d_status, true);
  if (rc || count == 0) return rc;
  return enqueue_inflate_batch(ctx, count, d_srcs, src_n, d_index, d_subindex, d_dsts, dst_n, block_bytes, container, d_status,
                               nullptr, stream ? (hipStream_t)stream : ctx->stream);
}

int sfh_decompress_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, const uint64_t* index,
                         const uint32_t* subindex, void* const* dsts, const uint64_t* dst_n, const uint32_t* block_bytes,
                         uint32_t container, uint32_t* status) {
  int rc = check_inflate_batch(ctx, count, srcs, src_n, index, subindex, dsts, dst_n, block_bytes, container, status, false);
  if (rc || count == 0) return rc;
  size_t segs = 0;
  for (size_t i = 0; i < count; ++i) segs += chunks_of((size_t)dst_n[i]);
  const size_t ix_bytes = (segs + count) * sizeof(uint64_t), sub_bytes = segs * SFH_SUBINDEX_WORDS * sizeof(uint32_t);
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, dst_n))) return rc;
  if (index) rc = ctx->d_index.grow(ctx, segs + count, "index staging");
  if (!rc && subindex) rc = ctx->d_sub.grow(ctx, segs * SFH_SUBINDEX_WORDS, "sub-index staging");
  if (!rc) rc = ensure_bstatus(ctx, count);
  if (rc) return rc;
  if (index) SF_HIP(hipMemcpyAsync(ctx->d_index, index, ix_bytes, hipMemcpyHostToDevice, s), "H2D index");
  if (subindex) SF_HIP(hipMemcpyAsync(ctx->d_sub, subindex, sub_bytes, hipMemcpyHostToDevice, s), "H2D sub-index");
  if ((rc = enqueue_inflate_batch(ctx, count, B.d_srcs.data(), src_n, index ? ctx->d_index.p : nullptr, subindex ? ctx->d_sub.p : nullptr,
                                  B.d_dsts.data(), dst_n, block_bytes, container, ctx->bstatus.d, nullptr, s)) != SFH_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if ((rc = read_bstatus(ctx, count, status, s))) return rc;
  return staged_down(ctx, B, count, dsts, dst_n, status);
}

int sfh_decompress_ranges_device_async(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                                       const uint32_t* d_subindex, size_t nseg, uint64_t total_n, uint32_t block_bytes,
                                       size_t count, const uint64_t* offsets, const uint64_t* lengths, void* const* d_dsts,
                                       uint32_t* d_status, void* stream) {
  int rc = check_ranges(ctx, d_src, d_index, d_subindex, nseg, total_n, block_bytes, count, offsets, lengths, d_dsts, d_status, true);
  if (rc || count == 0) return rc;
  sf::range::Plan P;
  if ((rc = plan_ranges_checked(ctx, total_n, block_bytes, count, offsets, lengths, P)) != SFH_OK) return rc;
  std::vector<RangeSource> from;
  try {
    from.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t r = 0; r < count; ++r) {
    const uint64_t g = P.spans[r].first_seg;
    from[r] = RangeSource{(const uint8_t*)d_src, src_n, d_index + g, d_subindex ? d_subindex + g * SFH_SUBINDEX_WORDS : nullptr};
  }
  return enqueue_ranges(ctx, P, from.data(), d_dsts, count, d_subindex != nullptr, d_status, stream ? (hipStream_t)stream : ctx->stream);
}

int sfh_decompress_range_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                                const uint32_t* d_subindex, size_t nseg, uint64_t total_n, uint32_t block_bytes,
                                uint64_t offset, uint64_t length, void* d_dst, uint32_t* status, void* stream) {
  if (!ctx || !status) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  void* dsts[1] = {d_dst};
  uint32_t aligned_status = 0;  // (stands in for the device status word in the argument check)
  int rc = check_ranges(ctx, d_src, d_index, d_subindex, nseg, total_n, block_bytes, 1, &offset, &length, dsts, &aligned_status, true);
  if (rc) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s)) || (rc = ensure_bstatus(ctx, 1))) return rc;
  rc = sfh_decompress_ranges_device_async(ctx, d_src, src_n, d_index, d_subindex, nseg, total_n, block_bytes, 1, &offset, &length,
                                          dsts, ctx->bstatus.d, s);
  if (rc || (rc = read_bstatus(ctx, 1, status, s))) return rc;
  if (*status) snprintf(ctx->err, sizeof ctx->err, "range [%llu, +%llu): DecompressStatus %u", (unsigned long long)offset,
                        (unsigned long long)length, *status);
  return SFH_OK;
}

int sfh_decompress_ranges(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* index, const uint32_t* subindex,
                          size_t nseg, uint64_t total_n, uint32_t block_bytes, size_t count, const uint64_t* offsets,
                          const uint64_t* lengths, void* const* dsts, uint32_t* status) {
  int rc = check_ranges(ctx, src, index, subindex, nseg, total_n, block_bytes, count, offsets, lengths, dsts, status, false);
  if (rc || count == 0) return rc;
  sf::range::Plan P;
  if ((rc = plan_ranges_checked(ctx, total_n, block_bytes, count, offsets, lengths, P)) != SFH_OK) return rc;
  // The items are the decode spans: each one's piece of the stream (sf::range::source_piece), and behind them, through the
  // same staging, its index entries and its sub-index words -- a span's rows are consecutive segments, so both are one slice
  // from first_seg on (`piece`, `len`, `off`: the pieces of one upload after the other).
  std::vector<sf::range::Piece> pc;
  std::vector<const void*> piece;
  std::vector<uint64_t> len, off;
  std::vector<RangeSource> from;
  try {
    pc.resize(count);
    piece.resize(count);
    len.resize(count);
    off.resize(count + 1);
    from.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t r = 0; r < count; ++r) {
    pc[r] = sf::range::source_piece(P.spans[r], index, src_n);
    piece[r] = (const uint8_t*)src + pc[r].lo;
    len[r] = pc[r].n;
  }
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, piece.data(), len.data(), lengths))) return rc;
  for (size_t r = 0; r < count; ++r) {
    const sf::range::Span& S = P.spans[r];
    piece[r] = index + S.first_seg;
    len[r] = S.nrows ? (S.nrows + 1) * sizeof(uint64_t) : 0;
    off[r + 1] = off[r] + len[r];
  }
  const size_t sub_bytes = P.rows.size() * SFH_SUBINDEX_WORDS * sizeof(uint32_t);
  rc = ctx->d_index.grow(ctx, std::max<uint64_t>(1, off[count] / sizeof(uint64_t)), "index staging");
  if (!rc && subindex) rc = ctx->d_sub.grow(ctx, std::max<size_t>(1, P.rows.size()) * SFH_SUBINDEX_WORDS, "sub-index staging");
  if (!rc) rc = ensure_bstatus(ctx, count);
  if (!rc) rc = stage_up(ctx, ctx->d_index, piece.data(), len.data(), off.data(), count, off[count], s);
  if (rc) return rc;
  for (size_t r = 0; r < count; ++r) {
    // (the base points pc[r].lo bytes in front of the piece: base + an index entry of the span is the uploaded byte)
    const uint8_t* base = (const uint8_t*)((uintptr_t)B.d_srcs[r] - (uintptr_t)pc[r].lo);
    const size_t row0 = (size_t)P.spans[r].row0 * SFH_SUBINDEX_WORDS;  // the span's first sub-index word in d_sub
    from[r] = RangeSource{base, pc[r].lo + pc[r].n, ctx->d_index + off[r] / sizeof(uint64_t), subindex ? ctx->d_sub + row0 : nullptr};
  }
  if (subindex) {
    for (size_t r = 0; r < count; ++r) {
      const sf::range::Span& S = P.spans[r];
      piece[r] = subindex + S.first_seg * SFH_SUBINDEX_WORDS;
      len[r] = (uint64_t)S.nrows * SFH_SUBINDEX_WORDS * sizeof(uint32_t);
      off[r] = (uint64_t)S.row0 * SFH_SUBINDEX_WORDS * sizeof(uint32_t);
    }
    if ((rc = stage_up(ctx, ctx->d_sub, piece.data(), len.data(), off.data(), count, sub_bytes, s))) return rc;
  }
  if ((rc = enqueue_ranges(ctx, P, from.data(), B.d_dsts.data(), count, subindex != nullptr, ctx->bstatus.d, s)) != SFH_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if ((rc = read_bstatus(ctx, count, status, s))) return rc;
  return staged_down(ctx, B, count, dsts, lengths, status);
}

uint32_t sfh_last_block_bytes(const sfh_ctx* ctx) { return (ctx && ctx->index_valid) ? ctx->last_block_bytes : 0u; }

size_t sfh_index_entries(const sfh_ctx* ctx) { return (ctx && ctx->index_valid) ? (size_t)ctx->last_chunks + 1 : 0; }

int sfh_copy_index(sfh_ctx* ctx, uint64_t* dst, size_t entries, int dst_on_device, void* stream) {
  if (!ctx || !dst || !ctx->index_valid || entries != (size_t)ctx->last_chunks + 1)
    return fail(ctx, SFH_E_INVALID_ARG, "index: no compress call yet, or entries != segments + 1", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  if (int rc = order_behind_last_call(ctx, s)) return rc;  // the index is written by the last call's k_scan, maybe on another stream
  SF_HIP(hipMemcpyAsync(dst, ctx->ws.offsets, entries * sizeof(uint64_t),
                        dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s), "copy index");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

int sfh_copy_subindex(sfh_ctx* ctx, uint32_t* dst, size_t words, int dst_on_device, void* stream) {
  if (!ctx || !dst || !ctx->index_valid || words != (size_t)ctx->last_chunks * SFH_SUBINDEX_WORDS)
    return fail(ctx, SFH_E_INVALID_ARG, "sub-index: no compress call yet, or words != segments * 64", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  if (int rc = order_behind_last_call(ctx, s)) return rc;  // written by the last call's k_emit
  SF_HIP(hipMemcpyAsync(dst, ctx->ws.subidx, words * sizeof(uint32_t),
                        dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s), "copy sub-index");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

int sfh_decompress_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                          const uint32_t* d_subindex, size_t nseg, void* d_dst, size_t dst_n, uint32_t block_bytes,
                          uint32_t* status, void* stream) {
  if (!ctx || !d_src || !d_index || !status || (!d_dst && dst_n)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_index & 7) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_subindex & 3))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, index 8, dst 16, sub-index 4)", hipSuccess);
  if (dst_n > ((size_t)1 << 44) || nseg != (size_t)chunks_of(dst_n))
    return fail(ctx, SFH_E_INVALID_ARG, "nseg != ceil(dst_n / 32768)", hipSuccess);
  if (block_bytes % sf::kChunk || block_bytes > sf::kMaxStrip)
    return fail(ctx, SFH_E_INVALID_ARG, "block_bytes: a multiple of 32768 up to 16 MiB (0 = 32768)", hipSuccess);
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // a batch of one raw item: its status and first failing segment land in d_value[0..1]
  const void* const srcs[1] = {d_src};
  void* const dsts[1] = {d_dst};
  const uint64_t src_ns[1] = {src_n}, dst_ns[1] = {dst_n};
  if (int rc = enqueue_inflate_batch(ctx, 1, srcs, src_ns, d_index, d_subindex, dsts, dst_ns, &block_bytes, 0, ctx->d_value,
                                     ctx->d_value + 1, s))
    return rc;
  return read_decode_status(ctx, status, s);
}

int sfh_decompress(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* index, const uint32_t* subindex,
                   size_t nseg, void* dst, size_t dst_n, uint32_t block_bytes, uint32_t* status) {
  if (!ctx || !src || !index || !status || (!dst && dst_n)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  const size_t ix_bytes = (nseg + 1) * sizeof(uint64_t), sub_bytes = nseg * SFH_SUBINDEX_WORDS * sizeof(uint32_t);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = ctx->d_index.grow(ctx, nseg + 1, "index staging");
  if (!rc && subindex) rc = ctx->d_sub.grow(ctx, nseg * SFH_SUBINDEX_WORDS, "sub-index staging");
  if (!rc) rc = host_up(ctx, src, src_n, dst_n);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  SF_HIP(hipMemcpyAsync(ctx->d_index, index, ix_bytes, hipMemcpyHostToDevice, s), "H2D index");
  if (subindex) SF_HIP(hipMemcpyAsync(ctx->d_sub, subindex, sub_bytes, hipMemcpyHostToDevice, s), "H2D sub-index");
  rc = sfh_decompress_device(ctx, ctx->d_in, src_n, ctx->d_index, subindex ? ctx->d_sub.p : nullptr, nseg, ctx->d_out,
                             dst_n, block_bytes, status, s);
  if (rc) return rc;
  return *status ? SFH_OK : host_down(ctx, dst, dst_n);
}

// ---- the dictzip table read back (sf_dz_plan.h) ----
int sfh_dz_read_index(const void* src, size_t src_n, sfh_dz_info* info, uint64_t* index, size_t index_cap) {
  if (!info || (!src && src_n) || (!index && index_cap)) return SFH_E_INVALID_ARG;
  sf::dz::Head H;
  const int rc = sf::dz::read_index((const uint8_t*)src, src_n, H, index, index_cap);
  if (rc != sf::dz::kOk) return rc;  // SFH_E_NOT_INDEXABLE, SFH_E_DST_TOO_SMALL: nothing written
  const bool ok = H.status == sf::dz::kStOk;
  *info = sfh_dz_info{ok ? H.total_n : 0, ok ? H.nseg : 0u, ok ? H.header_bytes : 0u, H.status, 0u};
  return SFH_OK;
}

int sfh_dz_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_dz_info* info, uint64_t* d_index, size_t index_cap,
                             void* stream) {
  if (!ctx || !info || (!d_src && src_n) || (!d_index && index_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_index & 7)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, index 8)", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  if (int rc = ctx->d_dzinfo.grow(ctx, 1, "dictzip info slot")) return rc;
  if (int rc = order_behind_last_call(ctx, s)) return rc;  // (the info slot is the context's)
  SF_HIP(sf::launch_dz_index((const uint8_t*)d_src, src_n, d_index, index_cap, ctx->d_dzinfo, s), "launch k_dz_index");
  sf::DzInfo r{};
  SF_HIP(hipMemcpyAsync(&r, ctx->d_dzinfo, sizeof r, hipMemcpyDeviceToHost, s), "copy dictzip info");
  if (int rc = mark_call_end(ctx, s)) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  if (r.rc == SFH_E_NOT_INDEXABLE) return fail(ctx, SFH_E_NOT_INDEXABLE, "no dictzip table of 32 KiB chunks in the gzip header", hipSuccess);
  if (r.rc == SFH_E_DST_TOO_SMALL) return fail(ctx, SFH_E_DST_TOO_SMALL, "index_cap < nseg + 1", hipSuccess);
  *info = sfh_dz_info{r.total_n, r.nseg, r.header_bytes, r.status, 0u};
  return SFH_OK;
}

int sfh_decompress_dz_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                             uint32_t* status, void* stream) {
  if (!ctx || (!d_src && src_n) || !dst_n_out || !status || (!d_dst && dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 15)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  const size_t entries = (size_t)SFH_DZ_MAX_CHUNKS + 1;
  if (int rc = ctx->d_index.grow(ctx, entries, "index staging")) return rc;
  sfh_dz_info info{};
  if (int rc = sfh_dz_read_index_device(ctx, d_src, src_n, &info, ctx->d_index, entries, s)) return rc;
  *dst_n_out = 0;
  *status = info.status;
  if (info.status) {
    snprintf(ctx->err, sizeof ctx->err, "dictzip header: DecompressStatus %u", info.status);
    return SFH_OK;
  }
  if (info.total_n > dst_cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "ISIZE above dst_cap", hipSuccess);
  // one gzip item with that index: the wrapper, ISIZE and the CRC-32 are sfh_decompress_batch's
  const void* const srcs[1] = {d_src};
  void* const dsts[1] = {d_dst};
  const uint64_t src_ns[1] = {src_n}, dst_ns[1] = {info.total_n};
  const uint32_t bb = sf::kChunk;
  if (int rc = enqueue_inflate_batch(ctx, 1, srcs, src_ns, ctx->d_index, nullptr, dsts, dst_ns, &bb, SFH_GZIP, ctx->d_value,
                                     ctx->d_value + 1, s))
    return rc;
  if (int rc = read_decode_status(ctx, status, s)) return rc;
  if (*status == 0) *dst_n_out = info.total_n;
  return SFH_OK;
}

int sfh_decompress_dz(sfh_ctx* ctx, const void* src, size_t src_n, void* dst, uint64_t dst_cap, uint64_t* dst_n_out,
                      uint32_t* status) {
  if (!ctx || (!src && src_n) || !dst_n_out || !status || (!dst && dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  // the header on the host first: what to refuse, and how much output staging the call needs.  (parse_head is everything
  // but the sizes' sum: that check -- Error when they reach past the trailer -- is k_dz_index's, in the device call below)
  sf::dz::Head H;
  if (sf::dz::parse_head((const uint8_t*)src, src_n, H) != sf::dz::kOk)
    return fail(ctx, SFH_E_NOT_INDEXABLE, "no dictzip table of 32 KiB chunks in the gzip header", hipSuccess);
  if (H.status != sf::dz::kStOk) {  // a header that does not parse: nothing goes up
    *status = H.status;
    *dst_n_out = 0;
    snprintf(ctx->err, sizeof ctx->err, "dictzip header: DecompressStatus %u", H.status);
    return SFH_OK;
  }
  if (H.total_n > dst_cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "ISIZE above dst_cap", hipSuccess);
  const uint64_t out_n = H.total_n;
  int rc = host_up(ctx, src, src_n, out_n);
  if (!rc) rc = sfh_decompress_dz_device(ctx, ctx->d_in, src_n, ctx->d_out, out_n, dst_n_out, status, ctx->stream);
  if (rc) return rc;
  return *status ? SFH_OK : host_down(ctx, dst, out_n);
}

int sfh_decompress_dz_ranges(sfh_ctx* ctx, const void* src, size_t src_n, size_t count, const uint64_t* offsets,
                             const uint64_t* lengths, void* const* dsts, uint32_t* status) {
  if (!ctx || (!src && src_n) || (count && !status)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  sf::dz::Head H;
  if (sf::dz::parse_head((const uint8_t*)src, src_n, H) != sf::dz::kOk)
    return fail(ctx, SFH_E_NOT_INDEXABLE, "no dictzip table of 32 KiB chunks in the gzip header", hipSuccess);
  std::vector<uint64_t> index;
  if (H.status == sf::dz::kStOk) {
    try {
      index.resize((size_t)H.nseg + 1);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
    }
    (void)sf::dz::read_index((const uint8_t*)src, src_n, H, index.data(), index.size());  // (H.status: the sizes' sum as well)
  }
  if (H.status != sf::dz::kStOk) {  // a table that does not parse: every range's status
    for (size_t r = 0; r < count; ++r) status[r] = H.status;
    snprintf(ctx->err, sizeof ctx->err, "dictzip header: DecompressStatus %u", H.status);
    return SFH_OK;
  }
  return sfh_decompress_ranges(ctx, src, src_n, index.data(), nullptr, H.nseg, H.total_n, sf::kChunk, count, offsets, lengths, dsts,
                               status);
}

// ---- BGZF, the reader (sf_bgzf_plan.h, sf_bgzf.hip) ----
int sfh_bgzf_read_index(const void* src, size_t src_n, sfh_bgzf_info* info, uint64_t* member_off, uint64_t* out_off, size_t cap) {
  if (!info || (!src && src_n) || ((!member_off || !out_off) && cap)) return SFH_E_INVALID_ARG;
  sf::bgzf::Info I;
  const int rc = sf::bgzf::read_index((const uint8_t*)src, src_n, I, member_off, out_off, cap);
  *info = sfh_bgzf_info{I.total_n, I.members, I.max_isize, I.has_eof, I.status};
  return rc;  // SFH_OK, SFH_E_DST_TOO_SMALL
}

namespace {
// the nodes of the file counted (one synchronisation); their per-workgroup offsets stay in ctx->d_bgzfcnt for the walk
int bgzf_count_nodes(sfh_ctx* ctx, const uint8_t* d_src, size_t src_n, hipStream_t s, uint32_t* nn) {
  const uint32_t nb = sf::bgzf_scan_blocks(src_n);
  const size_t words = 2 * (size_t)nb + sf::any_scan_tmp_words(nb) + 1;
  if (int rc = ctx->d_bgzfcnt.grow(ctx, words, "BGZF scan counts")) return rc;
  if (int rc = ctx->d_bgzfinfo.grow(ctx, 1, "BGZF info slot")) return rc;
  uint32_t* cnt = ctx->d_bgzfcnt;
  uint32_t *off = cnt + nb, *tmp = off + nb, *total = tmp + sf::any_scan_tmp_words(nb);
  if (int rc = order_behind_last_call(ctx, s)) return rc;
  SF_HIP(sf::launch_bgzf_count(d_src, src_n, cnt, s), "launch k_bgzf_scan");
  SF_HIP(sf::launch_scan_u32(cnt, off, nb, tmp, total, s), "scan of the node counts");
  SF_HIP(hipMemcpyAsync(nn, total, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "copy node count");
  if (int rc = mark_call_end(ctx, s)) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}
// ... and walked (one synchronisation): *r the info, member_off / out_off written when the file parses and cap holds them
int bgzf_walk_nodes(sfh_ctx* ctx, const uint8_t* d_src, size_t src_n, uint32_t nn, uint64_t* d_member_off, uint64_t* d_out_off,
                    size_t cap, hipStream_t s, sf::BgzfInfo* r) {
  if (int rc = ctx->d_bgzfwalk.grow(ctx, sf::bgzf_walk_bytes(nn), "BGZF walk scratch")) return rc;
  const uint32_t* off = ctx->d_bgzfcnt + sf::bgzf_scan_blocks(src_n);
  SF_HIP(sf::launch_bgzf_walk(d_src, src_n, off, nn, ctx->d_bgzfwalk, d_member_off, d_out_off, cap, ctx->d_bgzfinfo, s), "BGZF walk");
  SF_HIP(hipMemcpyAsync(r, ctx->d_bgzfinfo, sizeof *r, hipMemcpyDeviceToHost, s), "copy BGZF info");
  if (int rc = mark_call_end(ctx, s)) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}
}  // namespace

int sfh_bgzf_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_bgzf_info* info, uint64_t* d_member_off,
                               uint64_t* d_out_off, size_t cap, void* stream) {
  if (!ctx || !info || (!d_src && src_n) || ((!d_member_off || !d_out_off) && cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_member_off & 7) || ((uintptr_t)d_out_off & 7))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, index arrays 8)", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  *info = sfh_bgzf_info{0, 0, 0, 0, 0};
  if (src_n == 0) {  // no members
    if (!cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < members + 1", hipSuccess);
    const uint64_t zero = 0;
    SF_HIP(hipMemcpyAsync(d_member_off, &zero, sizeof zero, hipMemcpyHostToDevice, s), "index");
    SF_HIP(hipMemcpyAsync(d_out_off, &zero, sizeof zero, hipMemcpyHostToDevice, s), "index");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    return SFH_OK;
  }
  uint32_t nn = 0;
  if (int rc = bgzf_count_nodes(ctx, (const uint8_t*)d_src, src_n, s, &nn)) return rc;
  sf::BgzfInfo r{};
  if (int rc = bgzf_walk_nodes(ctx, (const uint8_t*)d_src, src_n, nn, d_member_off, d_out_off, cap, s, &r)) return rc;
  *info = sfh_bgzf_info{r.total_n, r.members, r.max_isize, r.has_eof, r.status};
  if (r.rc == SFH_E_DST_TOO_SMALL) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < members + 1", hipSuccess);
  return SFH_OK;
}

namespace {
// sfh_decompress_bgzf_device (widest = kChunk) and sfh_decompress_bgzf_wide_device (kWideRow): a file with a member above
// `widest` bytes is refused.  A file whose members all fit kChunk takes the narrow rows whichever call it came through; one
// with a member above that is decoded on wide rows as a whole: tokens kWideRow apart (so a launch batch holds half as many
// members and the token scratch keeps its bound), two checksum partials per member.
int bgzf_decode_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                       uint32_t* status, void* stream, uint32_t widest) {
  if (!ctx || (!d_src && src_n) || !dst_n_out || !status || (!d_dst && dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 15)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
  *dst_n_out = 0;
  *status = 0;
  if (src_n == 0) return SFH_OK;
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  // the index, in the context's own arrays: the file has no more members than nodes
  uint32_t nn = 0;
  if (int rc = bgzf_count_nodes(ctx, (const uint8_t*)d_src, src_n, s, &nn)) return rc;
  const size_t cap = (size_t)nn + 1;
  if (int rc = ctx->d_bgzfix.grow(ctx, 2 * cap, "BGZF index")) return rc;
  uint64_t *member_off = ctx->d_bgzfix, *out_off = ctx->d_bgzfix + cap;
  sf::BgzfInfo r{};
  if (int rc = bgzf_walk_nodes(ctx, (const uint8_t*)d_src, src_n, nn, member_off, out_off, cap, s, &r)) return rc;
  if (r.status) {
    *status = r.status;
    snprintf(ctx->err, sizeof ctx->err, "BGZF members: DecompressStatus %u", r.status);
    return SFH_OK;
  }
  if (r.max_isize > widest)
    return fail(ctx, SFH_E_NOT_INDEXABLE,
                widest == sf::kChunk ? "a BGZF member above 32768 bytes (sfh_decompress_bgzf_wide_device and sfh_decompress_bgzf read such files)"
                                     : "a member above 65536 bytes: not BGZF", hipSuccess);
  const bool wide = r.max_isize > sf::kChunk;
  if (r.total_n > dst_cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "the members' ISIZEs above dst_cap", hipSuccess);
  // every member one index-free gzip item of one segment; the rows are written on the device, from the device's index
  const uint32_t m = r.members, per = wide ? sf::bgzf::wide_batch(ctx->batch_chunks) : ctx->batch_chunks;
  if (wide && m > 0x7FFFFFFFu) return fail(ctx, SFH_E_INVALID_ARG, "2^31 members or more", hipSuccess);
  const uint32_t row = wide ? sf::kWideRow : sf::kChunk, nsums = (uint32_t)sf::bgzf::checksum_rows(m, wide);
  Carve L;
  const size_t o_segs = L.add<sf::InflateSeg>(m), o_items = L.add<sf::InflateItem>(m), o_clips = L.add<sf::InflateClip>(m);
  const size_t o_sums = L.add<sf::BatchChunk>(nsums), o_implied = L.add<uint64_t>(2 * (size_t)m), o_strips = L.add<sf::InflateStrip>(m);
  const size_t o_status = L.add<uint32_t>(m);
  int rc = ctx->d_bgzfrows.grow(ctx, L.bytes(), "BGZF decoder rows");
  if (!rc) rc = ensure_seginfo(ctx, (size_t)m);
  if (!rc) rc = ensure_dtok(ctx, std::min(m, per) * (row / sf::kChunk));
  if (!rc) rc = ensure_sums(ctx, nsums);
  if (rc) return rc;
  uint8_t* R = ctx->d_bgzfrows;
  sf::InflateSeg* segs = Carve::at<sf::InflateSeg>(R, o_segs);
  sf::InflateItem* items = Carve::at<sf::InflateItem>(R, o_items);
  sf::InflateClip* clips = Carve::at<sf::InflateClip>(R, o_clips);
  sf::BatchChunk* sums = Carve::at<sf::BatchChunk>(R, o_sums);
  uint64_t* implied = Carve::at<uint64_t>(R, o_implied);
  sf::InflateStrip* strips = Carve::at<sf::InflateStrip>(R, o_strips);
  uint32_t* d_status = Carve::at<uint32_t>(R, o_status);
  ctx->index_valid = false;
  ctx->bix_valid = false;
  ctx->ev_inf_valid = false;
  ctx->last_chunks = m;
  ctx->last_dtok_bytes = (size_t)std::min(m, per) * row * sizeof(uint32_t);
  if (wide)
    SF_HIP(sf::launch_bgzf_rows_wide((const uint8_t*)d_src, member_off, out_off, m, per, (uint8_t*)d_dst, segs, items, clips, strips, sums, implied, s),
           "launch k_bgzf_rows");
  else
    SF_HIP(sf::launch_bgzf_rows((const uint8_t*)d_src, member_off, out_off, m, per, (uint8_t*)d_dst, segs, items, clips, strips, sums, implied, s),
           "launch k_bgzf_rows");
  for (uint32_t b0 = 0; b0 < m; b0 += per) {
    const uint32_t nb = std::min(per, m - b0);
    sf::SegInfo* binfo = ctx->ws.seginfo + b0;
    if (wide) {
      SF_HIP(sf::launch_inflate_tokens_wide(segs + b0, nb, ctx->ws.tokens, binfo, !ctx->inflate_serial, s), "launch k_inflate_tokens");
      SF_HIP(sf::launch_inflate_bytes_wide(segs + b0, r.unaligned ? clips + b0 : nullptr, strips + b0, nb, ctx->ws.tokens, binfo, s),
             "launch k_inflate_bytes");
      continue;
    }
    SF_HIP(sf::launch_inflate_tokens(segs + b0, nb, ctx->ws.tokens, binfo, false, !ctx->inflate_serial, s), "launch k_inflate_tokens");
    // (a foreign file's ISIZEs may leave a member's output off a 16-byte boundary: the byte stage with a write window)
    if (r.unaligned) SF_HIP(sf::launch_inflate_bytes_clip(segs + b0, clips + b0, strips + b0, nb, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes_clip");
    else SF_HIP(sf::launch_inflate_bytes(segs + b0, strips + b0, nb, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes");
  }
  if (r.unaligned) SF_HIP(sf::launch_checksum_batch_any(sums, nsums, ctx->ws.sums, s), "launch k_checksum");
  else SF_HIP(sf::launch_checksum_batch(sums, nsums, SFH_GZIP, ctx->ws.sums, s), "launch k_checksum");
  if (wide) SF_HIP(sf::launch_inflate_fold_wide(items, m, ctx->ws.seginfo, ctx->ws.sums, SFH_GZIP, d_status, s), "launch k_inflate_fold");
  else SF_HIP(sf::launch_inflate_fold(items, m, ctx->ws.seginfo, ctx->ws.sums, SFH_GZIP, d_status, nullptr, s), "launch k_inflate_fold");
  SF_HIP(sf::launch_bgzf_first(d_status, m, ctx->d_value, s), "launch k_bgzf_first");
  uint32_t res[2] = {0, 0};
  SF_HIP(hipMemcpyAsync(res, ctx->d_value, sizeof res, hipMemcpyDeviceToHost, s), "copy status");
  if ((rc = mark_call_end(ctx, s))) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *status = res[0];
  if (res[0] == 0) *dst_n_out = r.total_n;
  else snprintf(ctx->err, sizeof ctx->err, "BGZF member %u: DecompressStatus %u", res[1], res[0]);
  return SFH_OK;
}
}  // namespace

int sfh_decompress_bgzf_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                               uint32_t* status, void* stream) {
  return bgzf_decode_device(ctx, d_src, src_n, d_dst, dst_cap, dst_n_out, status, stream, sf::kChunk);
}

int sfh_decompress_bgzf_wide_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                                    uint32_t* status, void* stream) {
  return bgzf_decode_device(ctx, d_src, src_n, d_dst, dst_cap, dst_n_out, status, stream, sf::kWideRow);
}

int sfh_decompress_bgzf(sfh_ctx* ctx, const void* src, size_t src_n, void* dst, uint64_t dst_cap, uint64_t* dst_n_out,
                        uint32_t* status) {
  if (!ctx || (!src && src_n) || !dst_n_out || !status || (!dst && dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  *dst_n_out = 0;
  *status = 0;
  // the members on the host first: what to refuse, which path, how much staging
  sf::bgzf::Info I;
  std::vector<uint64_t> member_off, out_off;
  if (sf::bgzf::read_index((const uint8_t*)src, src_n, I, nullptr, nullptr, 0) == sf::bgzf::kDstTooSmall) {
    try {
      member_off.resize((size_t)I.members + 1);
      out_off.resize((size_t)I.members + 1);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
    }
    (void)sf::bgzf::read_index((const uint8_t*)src, src_n, I, member_off.data(), out_off.data(), member_off.size());
  }
  if (I.status) {
    *status = I.status;
    snprintf(ctx->err, sizeof ctx->err, "BGZF members: DecompressStatus %u", I.status);
    return SFH_OK;
  }
  if (I.total_n > dst_cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "the members' ISIZEs above dst_cap", hipSuccess);
  if (I.members == 0) return SFH_OK;
  if (I.max_isize <= sf::kWideRow) {  // the device path: narrow rows, or wide ones for a file with a member above 32768 bytes
    const bool wide = I.max_isize > sf::kChunk;
    int rc = host_up(ctx, src, src_n, I.total_n);
    if (!rc) rc = bgzf_decode_device(ctx, ctx->d_in, src_n, ctx->d_out, I.total_n, dst_n_out, status, ctx->stream, wide ? sf::kWideRow : sf::kChunk);
    if (rc) return rc;
    return *status ? SFH_OK : host_down(ctx, dst, I.total_n);
  }
  // a member above 64 KiB (gzip members with BGZF's extra field, but not BGZF): each one an item of the stream decoder, into a
  // buffer of the call's own so that dst is written only when every member decoded
  const size_t m = I.members;
  std::vector<uint8_t> out;
  std::vector<const void*> srcs;
  std::vector<void*> dsts;
  std::vector<uint64_t> src_ns, caps, got;
  std::vector<uint32_t> st;
  try {
    out.resize(I.total_n ? I.total_n : 1);
    srcs.resize(m);
    dsts.resize(m);
    src_ns.resize(m);
    caps.resize(m);
    got.resize(m);
    st.resize(m);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t i = 0; i < m; ++i) {
    srcs[i] = (const uint8_t*)src + member_off[i];
    src_ns[i] = member_off[i + 1] - member_off[i];
    dsts[i] = out.data() + out_off[i];
    caps[i] = out_off[i + 1] - out_off[i];
  }
  if (int rc = sfh_inflate_stream_batch(ctx, m, srcs.data(), src_ns.data(), SFH_GZIP, dsts.data(), caps.data(), got.data(), st.data()))
    return rc;
  for (size_t i = 0; i < m; ++i) {
    const uint32_t sti = st[i] ? st[i] : (got[i] != caps[i] ? 1u : 0u);
    if (sti) {
      *status = sti;
      snprintf(ctx->err, sizeof ctx->err, "BGZF member %zu: DecompressStatus %u", i, sti);
      return SFH_OK;
    }
  }
  memcpy(dst, out.data(), I.total_n);
  *dst_n_out = I.total_n;
  return SFH_OK;
}

// ---- BGZF random access (sf_bgzf_range_plan.h; the kernels: sf_bgzf.hip) ----
namespace {
// Everything the calls check before they plan or enqueue anything (`dev`: device buffers and their alignment rules; the host
// call may come without an index, and then `info` is the host walk's).
int check_bgzf_ranges(sfh_ctx* ctx, const void* src, const uint64_t* member_off, const uint64_t* out_off, const sfh_bgzf_info* info,
                      size_t count, const uint64_t* offsets, const uint64_t* lengths, void* const* dsts, const uint32_t* status,
                      bool dev) {
  if (!src || !member_off || !out_off || !info || !offsets || !lengths || !dsts || !status)
    return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many ranges", hipSuccess);
  if (dev && (((uintptr_t)src & 3) || ((uintptr_t)member_off & 7) || ((uintptr_t)out_off & 7) || ((uintptr_t)status & 3)))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, index arrays 8, status 4)", hipSuccess);
  for (size_t r = 0; r < count; ++r) {
    if (!dsts[r] && lengths[r]) return fail(ctx, SFH_E_INVALID_ARG, "null destination", hipSuccess);
    if (offsets[r] > info->total_n || lengths[r] > info->total_n - offsets[r])
      return fail(ctx, SFH_E_INVALID_ARG, "a range ends behind total_n", hipSuccess);
  }
  if (int rc = check_disjoint(ctx, dsts, lengths, count)) return rc;
  if (info->max_isize > sf::kWideRow) return fail(ctx, SFH_E_NOT_INDEXABLE, "a member above 65536 bytes: not BGZF", hipSuccess);
  return SFH_OK;
}

// Device buffers, arguments checked; ranges[r]: the call's range rows (what each reads: the file itself, or the host call's
// per-span piece).  The rows go up in one copy; k_bgzf_range_spans and the scan plan on the device; the row total comes back
// (the planning synchronisation); then the row tables, the token kernels (as they are) and the clipped byte stage batch after
// batch, and the fold of every range's status.  Ends synchronised.
int enqueue_bgzf_ranges(sfh_ctx* ctx, const sf::BgzfRange* ranges, size_t count, const uint64_t* d_member_off, const uint64_t* d_out_off,
                        const sfh_bgzf_info* info, uint32_t* d_status, hipStream_t s) {
  const uint32_t n = (uint32_t)count;
  const bool wide = info->max_isize > sf::kChunk;
  const uint32_t row = wide ? sf::kWideRow : sf::kChunk, per = sf::bgzf::rows_per_batch(ctx->batch_chunks, wide);
  const size_t bytes = count * sizeof(sf::BgzfRange);
  // plan u32[2n] | row0 u32[n] | the scan's scratch and total | the rows' total (64-bit) | spans
  const size_t tmp_words = sf::any_scan_tmp_words(n);
  Carve G;
  const size_t o_plan = G.add<uint32_t>(2 * count), o_row0 = G.add<uint32_t>(count), o_tmp = G.add<uint32_t>(tmp_words + 1);
  const size_t o_total = G.add<uint64_t>(2), o_spans = G.add<sf::InflateSpan>(count);  // (the total: a slot of 16 bytes)
  int rc = ctx->tab.stage(ctx, bytes);
  if (!rc) rc = ctx->d_bgzfrng.grow(ctx, G.bytes(), "BGZF range plan");
  if (rc) return rc;
  memcpy(ctx->tab.h, ranges, bytes);
  const sf::BgzfRange* t_ranges = Carve::at<const sf::BgzfRange>(ctx->tab.d, 0);
  uint32_t* plan = Carve::at<uint32_t>(ctx->d_bgzfrng, o_plan);
  uint32_t* row0 = Carve::at<uint32_t>(ctx->d_bgzfrng, o_row0);
  uint32_t* tmp = Carve::at<uint32_t>(ctx->d_bgzfrng, o_tmp);
  unsigned long long* d_rows = Carve::at<unsigned long long>(ctx->d_bgzfrng, o_total);
  sf::InflateSpan* spans = Carve::at<sf::InflateSpan>(ctx->d_bgzfrng, o_spans);
  ctx->index_valid = false;
  ctx->bix_valid = false;
  ctx->ev_inf_valid = false;
  if ((rc = ctx->tab.upload(ctx, bytes, s)) != SFH_OK) return rc;
  SF_HIP(sf::launch_bgzf_range_spans(t_ranges, n, d_out_off, info->members, plan, d_rows, s), "launch k_bgzf_range_spans");
  SF_HIP(sf::launch_scan_u32(plan + n, row0, n, tmp, tmp + tmp_words, s), "scan of the ranges' rows");
  unsigned long long total = 0;
  SF_HIP(hipMemcpyAsync(&total, d_rows, sizeof total, hipMemcpyDeviceToHost, s), "copy row total");
  if ((rc = mark_call_end(ctx, s))) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  if (total > sf::bgzf::kMaxRangeRows) return fail(ctx, SFH_E_INVALID_ARG, "decode spans of more than 2^31 - 1 members in one call", hipSuccess);
  const uint32_t T = (uint32_t)total;
  const size_t t1 = std::max<size_t>(T, 1);
  Carve L;
  const size_t o_segs = L.add<sf::InflateSeg>(t1), o_clips = L.add<sf::InflateClip>(t1), o_strips = L.add<sf::InflateStrip>(t1);
  const size_t o_implied = L.add<uint64_t>(2 * t1), o_wst = L.add<uint32_t>(t1);
  rc = ctx->d_bgzfrows.grow(ctx, L.bytes(), "BGZF decoder rows");
  if (!rc) rc = ensure_seginfo(ctx, t1);
  if (!rc) rc = ensure_dtok(ctx, std::max(1u, std::min(T, per)) * (row / sf::kChunk));
  if (rc) return rc;
  uint8_t* R = ctx->d_bgzfrows;
  sf::InflateSeg* segs = Carve::at<sf::InflateSeg>(R, o_segs);
  sf::InflateClip* clips = Carve::at<sf::InflateClip>(R, o_clips);
  sf::InflateStrip* strips = Carve::at<sf::InflateStrip>(R, o_strips);
  uint64_t* implied = Carve::at<uint64_t>(R, o_implied);
  uint32_t* wst = Carve::at<uint32_t>(R, o_wst);
  ctx->last_chunks = T;
  ctx->last_dtok_bytes = (size_t)std::min(T, per) * row * sizeof(uint32_t);
  SF_HIP(sf::launch_bgzf_range_rows(t_ranges, n, d_member_off, d_out_off, plan, row0, T, per, row, segs, clips, strips, implied, wst, spans, s),
         "launch k_bgzf_range_rows");
  const uint64_t nbatches = sf::bgzf::range_batches(T, per);
  for (uint64_t b = 0; b < nbatches; ++b) {
    const size_t b0 = (size_t)(b * per);
    const uint32_t nb = sf::bgzf::range_batch_rows(T, per, b);
    sf::SegInfo* binfo = ctx->ws.seginfo + b0;
    if (wide) {
      SF_HIP(sf::launch_inflate_tokens_wide(segs + b0, nb, ctx->ws.tokens, binfo, !ctx->inflate_serial, s), "launch k_inflate_tokens");
      SF_HIP(sf::launch_inflate_bytes_wide(segs + b0, clips + b0, strips + b0, nb, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes_clip");
    } else {
      SF_HIP(sf::launch_inflate_tokens(segs + b0, nb, ctx->ws.tokens, binfo, false, !ctx->inflate_serial, s), "launch k_inflate_tokens");
      SF_HIP(sf::launch_inflate_bytes_clip(segs + b0, clips + b0, strips + b0, nb, ctx->ws.tokens, binfo, s), "launch k_inflate_bytes_clip");
    }
  }
  SF_HIP(sf::launch_bgzf_fold_spans(spans, n, plan, ctx->ws.seginfo, wst, d_status, s), "launch k_bgzf_fold_spans");
  if ((rc = mark_call_end(ctx, s))) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

// info->status != 0: every range's status, nothing decoded
int bgzf_ranges_all(sfh_ctx* ctx, uint32_t* d_status, size_t count, uint32_t st, hipStream_t s) {
  if (int rc = order_behind_last_call(ctx, s)) return rc;
  SF_HIP(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)st, count, s), "statuses");
  if (int rc = mark_call_end(ctx, s)) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  snprintf(ctx->err, sizeof ctx->err, "BGZF members: DecompressStatus %u", st);
  return SFH_OK;
}
}  // namespace

int sfh_decompress_bgzf_ranges_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_member_off,
                                      const uint64_t* d_out_off, const sfh_bgzf_info* info, size_t count, const uint64_t* offsets,
                                      const uint64_t* lengths, void* const* d_dsts, uint32_t* d_status, void* stream) {
  if (!ctx) return fail(ctx, SFH_E_INVALID_ARG, "argument (context)", hipSuccess);
  if (count == 0) return SFH_OK;
  int rc = check_bgzf_ranges(ctx, d_src, d_member_off, d_out_off, info, count, offsets, lengths, d_dsts, d_status, true);
  if (rc) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s))) return rc;
  if (info->status) return bgzf_ranges_all(ctx, d_status, count, info->status, s);
  std::vector<sf::BgzfRange> ranges;
  try {
    ranges.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t r = 0; r < count; ++r)
    ranges[r] = sf::BgzfRange{offsets[r], lengths[r], (uint8_t*)d_dsts[r], (const uint8_t*)d_src, 0, src_n};
  return enqueue_bgzf_ranges(ctx, ranges.data(), count, d_member_off, d_out_off, info, d_status, s);
}

int sfh_decompress_bgzf_ranges(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* member_off, const uint64_t* out_off,
                               const sfh_bgzf_info* info, size_t count, const uint64_t* offsets, const uint64_t* lengths,
                               void* const* dsts, uint32_t* status) {
  if (!ctx) return fail(ctx, SFH_E_INVALID_ARG, "argument (context)", hipSuccess);
  if (count == 0) return SFH_OK;
  const bool given = member_off || out_off || info;
  if (given && !(member_off && out_off && info)) return fail(ctx, SFH_E_INVALID_ARG, "member_off, out_off, info: all three or none", hipSuccess);
  if (!src || !status) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  // without an index: the members on the host first
  std::vector<uint64_t> w_moff, w_ooff;
  sfh_bgzf_info w_info{};
  if (!given) {
    sf::bgzf::Info I;
    (void)sf::bgzf::read_index((const uint8_t*)src, src_n, I, nullptr, nullptr, 0);  // the counts, or the status
    if (I.status) {  // a file that does not parse: every range's status, whatever the ranges are
      for (size_t r = 0; r < count; ++r) status[r] = I.status;
      snprintf(ctx->err, sizeof ctx->err, "BGZF members: DecompressStatus %u", I.status);
      return SFH_OK;
    }
    try {
      w_moff.resize((size_t)I.members + 1);
      w_ooff.resize((size_t)I.members + 1);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
    }
    (void)sf::bgzf::read_index((const uint8_t*)src, src_n, I, w_moff.data(), w_ooff.data(), w_moff.size());
    w_info = sfh_bgzf_info{I.total_n, I.members, I.max_isize, I.has_eof, I.status};
    member_off = w_moff.data();
    out_off = w_ooff.data();
    info = &w_info;
  }
  int rc = check_bgzf_ranges(ctx, src, member_off, out_off, info, count, offsets, lengths, dsts, status, false);
  if (rc) return rc;
  if (info->status) {  // (nothing goes up)
    for (size_t r = 0; r < count; ++r) status[r] = info->status;
    snprintf(ctx->err, sizeof ctx->err, "BGZF members: DecompressStatus %u", info->status);
    return SFH_OK;
  }
  // The items are the decode spans, planned here as the device plans them: each one's members' bytes (sf::bgzf::range_piece).
  const uint32_t m = info->members;
  std::vector<sf::bgzf::RangePiece> pc;
  std::vector<const void*> piece;
  std::vector<uint64_t> len;
  std::vector<sf::BgzfRange> ranges;
  try {
    pc.resize(count);
    piece.resize(count);
    len.resize(count);
    ranges.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  uint64_t rows = 0;
  for (size_t r = 0; r < count; ++r) {
    const sf::bgzf::Span S = sf::bgzf::span_of(out_off, m, offsets[r], lengths[r]);
    rows += S.rows;
    if (rows > sf::bgzf::kMaxRangeRows) return fail(ctx, SFH_E_INVALID_ARG, "decode spans of more than 2^31 - 1 members in one call", hipSuccess);
    pc[r] = sf::bgzf::range_piece(member_off, S, src_n);
    piece[r] = (const uint8_t*)src + pc[r].lo;
    len[r] = pc[r].n;
  }
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, piece.data(), len.data(), lengths))) return rc;
  const size_t ix_bytes = ((size_t)m + 1) * sizeof(uint64_t);
  rc = ctx->d_bgzfix.grow(ctx, 2 * ((size_t)m + 1), "BGZF index");
  if (!rc) rc = ensure_bstatus(ctx, count);
  if (rc) return rc;
  uint64_t *d_moff = ctx->d_bgzfix, *d_ooff = ctx->d_bgzfix + (size_t)m + 1;
  SF_HIP(hipMemcpyAsync(d_moff, member_off, ix_bytes, hipMemcpyHostToDevice, s), "H2D index");
  SF_HIP(hipMemcpyAsync(d_ooff, out_off, ix_bytes, hipMemcpyHostToDevice, s), "H2D index");
  for (size_t r = 0; r < count; ++r) {
    // (the base points pc[r].lo bytes in front of the piece: base + a member offset of the span is the uploaded byte)
    const uint8_t* base = (const uint8_t*)((uintptr_t)B.d_srcs[r] - (uintptr_t)pc[r].lo);
    ranges[r] = sf::BgzfRange{offsets[r], lengths[r], (uint8_t*)B.d_dsts[r], base, pc[r].lo, pc[r].lo + pc[r].n};
  }
  if ((rc = enqueue_bgzf_ranges(ctx, ranges.data(), count, d_moff, d_ooff, info, ctx->bstatus.d, s)) != SFH_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if ((rc = read_bstatus(ctx, count, status, s))) return rc;
  return staged_down(ctx, B, count, dsts, lengths, status);
}

int sfh_bgzf_voffsets_to_offsets(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, size_t count,
                                 const uint64_t* voffsets, uint64_t* offsets) {
  if (!member_off || !out_off || (count && (!voffsets || !offsets))) return SFH_E_INVALID_ARG;
  for (size_t k = 0; k < count; ++k) offsets[k] = sf::bgzf::voffset_to_offset(member_off, out_off, members, voffsets[k]);
  return SFH_OK;
}

int sfh_bgzf_offsets_to_voffsets(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, size_t count,
                                 const uint64_t* offsets, uint64_t* voffsets) {
  if (!member_off || !out_off || (count && (!offsets || !voffsets))) return SFH_E_INVALID_ARG;
  for (size_t k = 0; k < count; ++k) voffsets[k] = sf::bgzf::offset_to_voffset(member_off, out_off, members, offsets[k]);
  return SFH_OK;
}

// ---- ZIP archives (sf_zip_plan.h, sf_zip.hip) ----
static_assert(sizeof(sfh_zip_entry) == sizeof(sf::zip::Entry) && sizeof(sfh_zip_info) == sizeof(sf::zip::Info), "the plan's rows");

int sfh_zip_read_index(const void* src, size_t src_n, sfh_zip_info* info, sfh_zip_entry* entries, size_t cap) {
  if ((!src && src_n) || !info || (!entries && cap)) return SFH_E_INVALID_ARG;
  return sf::zip::read_index((const uint8_t*)src, src_n, *(sf::zip::Info*)info, (sf::zip::Entry*)entries, cap);
}

int sfh_zip_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_zip_info* info, sfh_zip_entry* entries, size_t cap,
                              void* stream) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if ((!d_src && src_n) || !info || (!entries && cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if ((uintptr_t)d_src & 3) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4)", hipSuccess);
  hipStream_t s;
  int rc = begin_call(ctx, stream, &s);
  if (rc) return rc;
  namespace z = sf::zip;
  z::Info& I = *(z::Info*)info;
  I = z::Info{0, 0, 0, 0, 0, z::kStOk};
  if (src_n < z::kEnd) {
    I.status = z::kStSrcTooSmall;
    return SFH_OK;
  }
  // (every return below that does not reach mark_call_end has either synchronised s or enqueued nothing on it)
  if ((rc = order_behind_last_call(ctx, s))) return rc;
  const uint8_t* file = (const uint8_t*)d_src;
  std::vector<uint8_t> buf;
  const size_t tail_n = std::min<size_t>(src_n, z::kTail);
  try {
    buf.resize(tail_n);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  SF_HIP(hipMemcpyAsync(buf.data(), file + (src_n - tail_n), tail_n, hipMemcpyDeviceToHost, s), "D2H the file's tail");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  z::End E;
  if (z::read_end(buf.data(), tail_n, src_n, E) != z::kStOk) {
    I.status = E.status;
    return SFH_OK;
  }
  const uint8_t* cd = nullptr;  // the directory: inside the tail already, or copied down
  if (E.cd_off >= src_n - tail_n) {
    cd = buf.data() + (E.cd_off - (src_n - tail_n));
  } else {
    try {
      buf.resize(E.cd_size);
    } catch (...) {
      return fail(ctx, SFH_E_NOMEM, "host memory for the directory", hipSuccess);
    }
    SF_HIP(hipMemcpyAsync(buf.data(), file + E.cd_off, E.cd_size, hipMemcpyDeviceToHost, s), "D2H the directory");
    SF_HIP(hipStreamSynchronize(s), "stream sync");
    cd = buf.data();
  }
  uint64_t total = 0;
  if (z::walk_central(cd, E.cd_size, E.cd_off, E.entries, nullptr, &total) != z::kStOk) {
    I.status = z::kStError;
    return SFH_OK;
  }
  I = z::Info{E.entries, E.cd_off, E.cd_size, total, E.zip64, z::kStOk};
  if (cap < E.entries) return SFH_E_DST_TOO_SMALL;
  if (E.entries == 0) return SFH_OK;
  z::walk_central(cd, E.cd_size, E.cd_off, E.entries, (z::Entry*)entries, &total);
  const size_t bytes = (size_t)E.entries * sizeof(z::Entry);
  if ((rc = ctx->d_zip.grow(ctx, bytes, "entry table"))) return rc;
  SF_HIP(hipMemcpyAsync(ctx->d_zip, entries, bytes, hipMemcpyHostToDevice, s), "H2D entry table");
  SF_HIP(sf::launch_zip_locals(file, E.cd_off, Carve::at<z::Entry>(ctx->d_zip, 0), E.entries, s), "launch k_zip_locals");
  SF_HIP(hipMemcpyAsync(entries, ctx->d_zip, bytes, hipMemcpyDeviceToHost, s), "D2H entry table");
  if ((rc = mark_call_end(ctx, s))) return rc;
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

namespace {
// The decode of `count` entries of a device file into device destinations, arguments checked; statuses on the host.
// Synchronises s.
int zip_decode(sfh_ctx* ctx, const uint8_t* file, uint64_t src_n, const sfh_zip_entry* entries, size_t count, void* const* d_dsts,
               const uint64_t* dst_cap, uint32_t* status, hipStream_t s) {
  namespace z = sf::zip;
  std::vector<sf::ZipCopy> copies;
  std::vector<sf::ZipPiece> pieces;
  std::vector<size_t> dfl;  // the deflated entries that go to the decoders, in call order
  ctx->any_ms[0] = ctx->any_ms[1] = 0;
  ctx->any_counts[0] = ctx->any_counts[1] = 0;
  for (float& m : ctx->stm_ms) m = 0;
  for (uint64_t& c : ctx->stm_counts) c = 0;
  int rc = SFH_OK;
  try {
    uint64_t segs = 0, waves = 0, sum_rows = 0;
    size_t live = 0;
    for (size_t i = 0; i < count; ++i) {
      const sfh_zip_entry& E = entries[i];
      uint32_t st = E.status;
      if (!st && E.method != 0 && E.method != 8) st = SFH_ZIP_ENTRY_UNSUPPORTED;
      if (!st && (E.data_off > src_n || E.csize > src_n - E.data_off)) st = z::kStSrcTooSmall;
      if (!st && E.method == 0 && E.csize != E.usize) st = z::kStError;
      if (!st && E.usize > 0xFFFFFFFFull) st = SFH_ZIP_ENTRY_UNSUPPORTED;  // (the CRC-32 fold counts an entry's bytes in 32 bits)
      if (!st && E.usize > dst_cap[i]) st = z::kStDstTooSmall;
      status[i] = st;
      if (st) continue;
      ++live;
      sum_rows += chunks_of((size_t)E.usize);
      if (E.method == 0) {
        const uint64_t np = (E.usize + z::kPiece - 1) / z::kPiece;
        if (np > 0xFFFFFFFFull || copies.size() >= 0xFFFFFFFFull) return fail(ctx, SFH_E_INVALID_ARG, "too many pieces", hipSuccess);
        for (uint64_t p = 0; p < np; ++p) pieces.push_back(sf::ZipPiece{(uint32_t)copies.size(), (uint32_t)p});
        copies.push_back(sf::ZipCopy{file + E.data_off, (uint8_t*)d_dsts[i], E.usize});
      } else {
        dfl.push_back(i);
        const uint32_t ns = chunks_of((size_t)E.usize);
        segs += ns;
        if (ns > 1) waves += ((E.data_off & 3) + E.csize + 8191) / 8192;
      }
    }
    if (pieces.size() > 0x7FFFFFFFull || sum_rows > 0x7FFFFFFFull || segs > ((uint64_t)1 << 31) - 1 || waves > ((uint64_t)1 << 31) - 1)
      return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 pieces, segments or scan waves in one call", hipSuccess);
    if ((rc = order_behind_last_call(ctx, s))) return rc;
    // one table for the call, sized before anything reads it: copy rows | piece rows | checksum rows | fold rows | statuses
    Carve L;
    const size_t o_copies = L.add<sf::ZipCopy>(copies.size()), o_pieces = L.add<sf::ZipPiece>(pieces.size());
    const size_t o_sums = L.add<sf::BatchChunk>((size_t)sum_rows), o_fold = L.add<sf::InflateItem>(live), o_st = L.add<uint32_t>(live);
    if (ctx->d_zip.cap < L.bytes() + 16 && (rc = wait_idle(ctx))) return rc;
    if ((rc = ctx->d_zip.grow(ctx, L.bytes() + 16, "ZIP decode rows"))) return rc;
    uint8_t* T = ctx->d_zip;
    // the stored entries: one gather copy (the rows are host vectors that live to the call's last synchronisation)
    if (!copies.empty()) {
      SF_HIP(hipMemcpyAsync(T + o_copies, copies.data(), copies.size() * sizeof(sf::ZipCopy), hipMemcpyHostToDevice, s), "H2D copy rows");
      SF_HIP(hipMemcpyAsync(T + o_pieces, pieces.data(), pieces.size() * sizeof(sf::ZipPiece), hipMemcpyHostToDevice, s), "H2D piece rows");
      SF_HIP(sf::launch_zip_store(Carve::at<const sf::ZipCopy>(T, o_copies), Carve::at<const sf::ZipPiece>(T, o_pieces), (uint32_t)pieces.size(),
                                  file, src_n, s), "launch k_zip_store");
    }
    // the deflated entries: an item is the 4-byte aligned part of the file around the entry's data, its body the data
    const size_t nd = dfl.size();
    if (nd) {
      std::vector<const void*> srcs(nd);
      std::vector<void*> dsts(nd);
      std::vector<uint64_t> sn(nd), un(nd), bodies(2 * nd), lead(nd), got(nd);
      std::vector<uint32_t> st(nd);
      for (size_t j = 0; j < nd; ++j) {
        const sfh_zip_entry& E = entries[dfl[j]];
        lead[j] = E.data_off & 3;
        srcs[j] = file + (E.data_off - lead[j]);
        sn[j] = lead[j] + E.csize;
        un[j] = E.usize;
        bodies[2 * j] = lead[j];
        bodies[2 * j + 1] = sn[j];
        dsts[j] = d_dsts[dfl[j]];
      }
      AnyBatch R;
      if ((rc = any_batch_recover(ctx, nd, srcs.data(), sn.data(), SFH_RAW, un.data(), un.data(), nullptr, s, R, bodies.data()))) return rc;
      if ((rc = any_batch_decode(ctx, nd, srcs.data(), sn.data(), SFH_RAW, dsts.data(), ctx->d_anyix, s, R))) return rc;
      // what the walk could not index: the stream decoder, with a capacity of usize.  An entry whose segments came up short
      // (SrcTooSmall: the index promised a segment more bytes than its blocks made) goes there as well -- a directory that states
      // more bytes than the body holds is such an entry -- and gets the serial decoder's word on the body as a whole: a body that
      // ends in order with other than usize bytes is Error, one that is cut short keeps SrcTooSmall.
      std::vector<size_t> rest;
      for (size_t j = 0; j < nd; ++j) {
        status[dfl[j]] = R.st[j];
        if (R.st[j] == SFH_ITEM_NOT_INDEXABLE || R.st[j] == z::kStSrcTooSmall) rest.push_back(j);
      }
      if (!rest.empty()) {
        const size_t nr = rest.size();
        uint64_t nc = 0;
        for (size_t k = 0; k < nr; ++k) {
          const size_t j = rest[k];
          srcs[k] = srcs[j];
          sn[k] = sn[j];
          un[k] = un[j];
          lead[k] = lead[j];
          dsts[k] = dsts[j];
          nc += (sn[k] + ctx->stream_chunk - 1) / ctx->stream_chunk + 1;
        }
        if (nc > ((uint64_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 nominal chunks (SFH_STREAM_CHUNK)", hipSuccess);
        if ((rc = stream_batch_run(ctx, nr, srcs.data(), sn.data(), SFH_RAW, dsts.data(), un.data(), false, nullptr, got.data(), st.data(),
                                   s, lead.data())))
          return rc;
        for (size_t k = 0; k < nr; ++k)
          status[dfl[rest[k]]] = st[k] ? st[k] : got[k] != un[k] ? z::kStError : 0u;
      }
    }
    // the CRC-32 of every entry that decoded: a partial per 32 KiB piece of its output, folded per entry against the directory's
    std::vector<sf::BatchChunk> sums;
    std::vector<sf::InflateItem> fold;
    std::vector<size_t> fold_entry;
    for (size_t i = 0; i < count; ++i) {
      if (status[i]) continue;
      const sfh_zip_entry& E = entries[i];
      const uint32_t np = chunks_of((size_t)E.usize);
      fold.push_back(sf::InflateItem{file, 0, E.usize, nullptr, nullptr, (uint32_t)sums.size(), 0, 0, E.crc32, (uint32_t)E.usize, 0});
      fold_entry.push_back(i);
      for (uint32_t p = 0; p < np; ++p) {
        const uint64_t ob = (uint64_t)p * sf::kChunk;
        // (an empty output: one empty row, at a real address)
        sums.push_back(sf::BatchChunk{E.usize ? (const uint8_t*)d_dsts[i] + ob : file, (uint32_t)std::min<uint64_t>(sf::kChunk, E.usize - ob), 0u});
      }
    }
    if (!fold.empty()) {
      if ((rc = ensure_sums(ctx, (uint32_t)sums.size()))) return rc;
      std::vector<uint32_t> fst(fold.size());
      SF_HIP(hipMemcpyAsync(T + o_sums, sums.data(), sums.size() * sizeof(sf::BatchChunk), hipMemcpyHostToDevice, s), "H2D checksum rows");
      SF_HIP(hipMemcpyAsync(T + o_fold, fold.data(), fold.size() * sizeof(sf::InflateItem), hipMemcpyHostToDevice, s), "H2D fold rows");
      SF_HIP(sf::launch_checksum_batch(Carve::at<const sf::BatchChunk>(T, o_sums), (uint32_t)sums.size(), SFH_GZIP, ctx->ws.sums, s), "launch k_checksum");
      SF_HIP(sf::launch_inflate_fold(Carve::at<const sf::InflateItem>(T, o_fold), (uint32_t)fold.size(), nullptr, ctx->ws.sums, SFH_GZIP,
                                     Carve::at<uint32_t>(T, o_st), nullptr, s), "launch k_inflate_fold");
      SF_HIP(hipMemcpyAsync(fst.data(), T + o_st, 4 * fold.size(), hipMemcpyDeviceToHost, s), "D2H checksums");
      if ((rc = mark_call_end(ctx, s))) return rc;
      SF_HIP(hipStreamSynchronize(s), "stream sync");
      for (size_t f = 0; f < fold.size(); ++f) status[fold_entry[f]] = fst[f];
    } else {
      if ((rc = mark_call_end(ctx, s))) return rc;
      SF_HIP(hipStreamSynchronize(s), "stream sync");
    }
  } catch (const std::bad_alloc&) {
    (void)hipStreamSynchronize(s);
    return fail(ctx, SFH_E_NOMEM, "host memory for the entry rows", hipSuccess);
  }
  ctx->index_valid = false;
  ctx->bix_valid = false;
  return SFH_OK;
}

int check_zip_decode(sfh_ctx* ctx, const void* src, size_t src_n, const sfh_zip_entry* entries, size_t count, void* const* dsts,
                     const uint64_t* dst_cap, const uint32_t* status, bool dev) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if (count == 0) return SFH_OK;
  if ((!src && src_n) || (dev && !entries) || !dsts || !dst_cap || !status) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many entries", hipSuccess);
  if (dev && ((uintptr_t)src & 3)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4)", hipSuccess);
  for (size_t i = 0; i < count; ++i) {
    if (!dsts[i] && dst_cap[i]) return fail(ctx, SFH_E_INVALID_ARG, "null destination", hipSuccess);
    if (dev && ((uintptr_t)dsts[i] & 15)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (dst 16)", hipSuccess);
  }
  return check_disjoint(ctx, dsts, dst_cap, count);
}
}  // namespace

int sfh_decompress_zip_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const sfh_zip_entry* entries, size_t count,
                              void* const* d_dsts, const uint64_t* dst_cap, uint32_t* status, void* stream) {
  int rc = check_zip_decode(ctx, d_src, src_n, entries, count, d_dsts, dst_cap, status, true);
  if (rc || count == 0) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s))) return rc;
  return zip_decode(ctx, (const uint8_t*)d_src, src_n, entries, count, d_dsts, dst_cap, status, s);
}

int sfh_decompress_zip(sfh_ctx* ctx, const void* src, size_t src_n, const sfh_zip_entry* entries, size_t count, void* const* dsts,
                       const uint64_t* dst_cap, uint32_t* status) {
  int rc = check_zip_decode(ctx, src, src_n, entries, count, dsts, dst_cap, status, false);
  if (rc || count == 0) return rc;
  std::vector<sfh_zip_entry> own;
  std::vector<uint64_t> off, slot, got;
  std::vector<void*> d_dsts;
  try {
    if (!entries) {  // walked here
      sfh_zip_info info;
      rc = sfh_zip_read_index(src, src_n, &info, nullptr, 0);
      if (rc == SFH_OK && info.status) {
        for (size_t i = 0; i < count; ++i) status[i] = info.status;
        return SFH_OK;
      }
      if (info.entries != count) return fail(ctx, SFH_E_INVALID_ARG, "count is not the archive's number of entries", hipSuccess);
      own.resize(count);
      if ((rc = sfh_zip_read_index(src, src_n, &info, own.data(), count))) return fail(ctx, rc, "sfh_zip_read_index", hipSuccess);
      entries = own.data();
    }
    off.resize(count + 1);
    slot.resize(count);
    got.resize(count);
    d_dsts.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  // every entry that can be decoded gets a slot of its size in the packed layout (sf_stage_plan.h); the others none
  for (size_t i = 0; i < count; ++i)
    slot[i] = (!entries[i].status && entries[i].usize <= dst_cap[i] && entries[i].usize <= 0xFFFFFFFFull) ? entries[i].usize : 0;
  sf::stage::pack_layout(slot.data(), count, off.data());
  if ((rc = host_up(ctx, src, src_n, (size_t)off[count]))) return rc;
  if ((rc = ctx->h_stage.grow(ctx, kStageBytes, "pinned staging"))) return rc;
  for (size_t i = 0; i < count; ++i) d_dsts[i] = ctx->d_out + off[i];
  if ((rc = zip_decode(ctx, ctx->d_in, src_n, entries, count, d_dsts.data(), slot.data(), status, ctx->stream))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  // (an entry without a slot: DstTooSmall against a capacity of 0 unless it had a status of its own; say what the caller's was)
  uint64_t end = 0;
  for (size_t i = 0; i < count; ++i) {
    got[i] = (dsts[i] && !status[i]) ? entries[i].usize : 0;
    if (got[i]) end = off[i] + got[i];
  }
  return stage_down(ctx, dsts, got.data(), off.data(), count, end, ctx->stream);
}

// ---- the writer ----
size_t sfh_zip_bound(size_t count, const uint64_t* src_n, const uint32_t* name_len) {
  if (count && (!src_n || !name_len)) return 0;
  return (size_t)sf::zip::bound(count, src_n, name_len);
}

namespace {
int check_zip_compress(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, const char* const* names,
                       const uint32_t* name_len, const void* dst, size_t cap, const void* out_n, const sfh_options* opt, bool dev) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if (check_opt(opt) || (opt && (opt->container != SFH_RAW || opt->final_stream != 1)))
    return fail(ctx, SFH_E_INVALID_ARG, "ZIP: container SFH_RAW, final_stream 1", hipSuccess);
  if (!dst || !out_n || (count && (!srcs || !src_n || !names || !name_len))) return fail(ctx, SFH_E_INVALID_ARG, "null array", hipSuccess);
  if (dev && ((uintptr_t)dst & 3)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (dst 4)", hipSuccess);
  if (count > ((size_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "too many items", hipSuccess);
  uint64_t chunks = 0, locals = 0, dir = 0;
  for (size_t i = 0; i < count; ++i) {
    if ((!srcs[i] && src_n[i]) || !names[i]) return fail(ctx, SFH_E_INVALID_ARG, "null item pointer", hipSuccess);
    if (dev && ((uintptr_t)srcs[i] & 15)) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 16)", hipSuccess);
    if (name_len[i] == 0 || name_len[i] > 65535) return fail(ctx, SFH_E_INVALID_ARG, "a name of 1 to 65535 bytes", hipSuccess);
    if (src_n[i] >= sf::zip::kMaxItem) return fail(ctx, SFH_E_INVALID_ARG, "an item of 2^32 - 1 bytes or more (ZIP64 sizes: out of scope)", hipSuccess);
    chunks += chunks_of((size_t)src_n[i]);
    locals += sf::zip::kLocal + name_len[i] + sf::zip::body_bound(src_n[i]);
    dir += sf::zip::kCentral + name_len[i];
    if (locals + dir >= ((uint64_t)1 << 32))
      return fail(ctx, SFH_E_INVALID_ARG, "the local parts' bounds and the directory reach 2^32 (ZIP64 offsets: out of scope)", hipSuccess);
  }
  if (chunks > ((uint64_t)1 << 31) - 1) return fail(ctx, SFH_E_INVALID_ARG, "more than 2^31 - 1 chunks in one call", hipSuccess);
  if (cap < sfh_zip_bound(count, src_n, name_len)) return fail(ctx, SFH_E_DST_TOO_SMALL, "cap < sfh_zip_bound", hipSuccess);
  return SFH_OK;
}

// Device buffers, arguments checked.  The tables -- item rows, the fold's rows, the pieces of every item's bound, the names -- are
// built in pinned memory and go up with one copy; then launch batch after launch batch: the batch call's kernels into the
// scratch slots (enqueue_batch, with the CRC-32 partials), the fold, the scan of the local parts, the pack; then the directory.
int enqueue_zip(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, const char* const* names,
                const uint32_t* name_len, uint8_t* d_dst, uint64_t* d_out_n, const sfh_options* opt, hipStream_t s) {
  namespace z = sf::zip;
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  (void)hipGetLastError();
  struct Group {
    size_t i0, i1, p0, p1;
    uint64_t slots;
  };
  std::vector<Group> groups;
  std::vector<sf::ZipItem> items;
  std::vector<sf::WrapItem> wraps;
  std::vector<sf::ZipPiece> pieces;
  std::vector<void*> slot_ptr;
  uint64_t names_n = 0, widest = 16;
  try {
    items.resize(count);
    wraps.resize(count);
    slot_ptr.resize(count);
    Group g{0, 0, 0, 0, 0};
    uint32_t gchunks = 0;
    auto close = [&](size_t i) {
      if (i > g.i0) {
        g.i1 = i;
        g.p1 = pieces.size();
        groups.push_back(g);
        widest = std::max(widest, g.slots);
      }
      g = Group{i, i, pieces.size(), pieces.size(), 0};
      gchunks = 0;
    };
    for (size_t i = 0; i < count; ++i) {
      const uint32_t nc = chunks_of((size_t)src_n[i]);
      if (gchunks && gchunks + nc > ctx->batch_chunks) close(i);
      const uint64_t b = z::body_bound(src_n[i]);
      items[i] = sf::ZipItem{names_n, g.slots, b, name_len[i], (uint32_t)src_n[i]};
      wraps[i] = sf::WrapItem{nullptr, src_n[i], (uint32_t)i, gchunks, nc, 0};
      for (uint64_t p = 0; p < (b + z::kPiece - 1) / z::kPiece; ++p) pieces.push_back(sf::ZipPiece{(uint32_t)i, (uint32_t)p});
      g.slots += b;  // (a multiple of 16: every slot starts 16-byte aligned)
      gchunks += nc;
      names_n += name_len[i];
    }
    close(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory for the descriptor tables", hipSuccess);
  }
  // uploaded: items | wraps | pieces | names; device only: out_n u64[count] | off u64[count] | carry u64 | crc u32[count]
  Carve L;
  const size_t o_items = L.add<sf::ZipItem>(count), o_wraps = L.add<sf::WrapItem>(count), o_pieces = L.add<sf::ZipPiece>(pieces.size());
  const size_t o_names = L.add<uint8_t>(names_n), up = L.bytes();
  const size_t o_outn = L.add<uint64_t>(count), o_off = L.add<uint64_t>(count), o_carry = L.add<uint64_t>(2), o_crc = L.add<uint32_t>(count);
  int rc = ctx->zipw.stage(ctx, up, L.bytes() + 16 - up);
  if (!rc && ctx->d_zipbody.cap < widest) rc = wait_idle(ctx);  // (the last call's kernels read it)
  if (!rc) rc = ctx->d_zipbody.grow(ctx, widest, "ZIP body scratch");
  if (rc) return rc;
  uint8_t* H = ctx->zipw.h;
  memcpy(H + o_items, items.data(), count * sizeof(sf::ZipItem));
  memcpy(H + o_wraps, wraps.data(), count * sizeof(sf::WrapItem));
  memcpy(H + o_pieces, pieces.data(), pieces.size() * sizeof(sf::ZipPiece));
  for (size_t i = 0; i < count; ++i) memcpy(H + o_names + items[i].name_off, names[i], name_len[i]);
  uint8_t* T = ctx->zipw.d;
  const sf::ZipItem* t_items = Carve::at<const sf::ZipItem>(T, o_items);
  const sf::WrapItem* t_wraps = Carve::at<const sf::WrapItem>(T, o_wraps);
  const sf::ZipPiece* t_pieces = Carve::at<const sf::ZipPiece>(T, o_pieces);
  uint64_t* t_outn = Carve::at<uint64_t>(T, o_outn);
  uint64_t* t_off = Carve::at<uint64_t>(T, o_off);
  uint64_t* t_carry = Carve::at<uint64_t>(T, o_carry);
  uint32_t* t_crc = Carve::at<uint32_t>(T, o_crc);
  if ((rc = up ? ctx->zipw.upload(ctx, up, s) : order_behind_last_call(ctx, s))) return rc;
  SF_HIP(hipMemsetAsync(t_carry, 0, 16, s), "clear the carry");
  if ((rc = mark_call_end(ctx, s))) return rc;  // (the batch calls below take their place behind this on s)
  for (const Group& g : groups) {
    const size_t n = g.i1 - g.i0;
    for (size_t i = g.i0; i < g.i1; ++i) slot_ptr[i] = ctx->d_zipbody + items[i].slot_off;
    if ((rc = enqueue_batch(ctx, n, d_srcs + g.i0, src_n + g.i0, slot_ptr.data() + g.i0, t_outn + g.i0, opt, s, true))) return rc;
    SF_HIP(sf::launch_crc_items(ctx->ws.sums, t_wraps + g.i0, (uint32_t)n, t_crc, s), "launch k_crc_items");
    SF_HIP(sf::launch_zip_place(t_items + g.i0, t_outn + g.i0, (uint32_t)n, t_off + g.i0, t_carry, s), "launch k_zip_place");
    SF_HIP(sf::launch_zip_pack(t_items, t_pieces + g.p0, (uint32_t)(g.p1 - g.p0), T + o_names, t_outn, t_off, t_crc, ctx->d_zipbody,
                               d_dst, s), "launch k_zip_pack");
  }
  SF_HIP(sf::launch_zip_wrap(t_items, T + o_names, t_outn, t_off, t_crc, count, names_n, t_carry, d_dst, d_out_n, s), "launch k_zip_wrap");
  ctx->index_valid = false;
  ctx->bix_valid = false;
  return mark_call_end(ctx, s);
}
}  // namespace

int sfh_compress_zip_device_async(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                  const char* const* names, const uint32_t* name_len, void* d_dst, size_t cap, uint64_t* d_out_n,
                                  const sfh_options* opt, void* stream) {
  const int rc = check_zip_compress(ctx, count, d_srcs, src_n, names, name_len, d_dst, cap, d_out_n, opt, true);
  if (rc) return rc;
  return enqueue_zip(ctx, count, d_srcs, src_n, names, name_len, (uint8_t*)d_dst, d_out_n, opt, stream ? (hipStream_t)stream : ctx->stream);
}

int sfh_compress_zip_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, const char* const* names,
                            const uint32_t* name_len, void* d_dst, size_t cap, size_t* out_n, const sfh_options* opt, void* stream) {
  int rc = check_zip_compress(ctx, count, d_srcs, src_n, names, name_len, d_dst, cap, out_n, opt, true);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  if ((rc = enqueue_zip(ctx, count, d_srcs, src_n, names, name_len, (uint8_t*)d_dst, ctx->d_total, opt, s))) return rc;
  SF_HIP(hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy size");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *out_n = (size_t)*ctx->h_total;
  return SFH_OK;
}

int sfh_compress_zip(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, const char* const* names,
                     const uint32_t* name_len, void* dst, size_t cap, size_t* out_n, const sfh_options* opt) {
  int rc = check_zip_compress(ctx, count, srcs, src_n, names, name_len, dst, cap, out_n, opt, false);
  if (rc) return rc;
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, nullptr))) return rc;
  if ((rc = ctx->d_out.grow(ctx, sfh_zip_bound(count, src_n, name_len), "output staging"))) return rc;
  if ((rc = enqueue_zip(ctx, count, B.d_srcs.data(), src_n, names, name_len, ctx->d_out, ctx->d_total, opt, s))) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  SF_HIP(hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "copy size");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  *out_n = (size_t)*ctx->h_total;
  return host_down(ctx, dst, *out_n);
}

int sfh_recover_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, uint64_t dst_n, uint64_t* d_index,
                             size_t nseg, uint8_t* d_depends, void* stream) {
  if (int rc = check_any(ctx, d_src, src_n, container, dst_n, true)) return rc;
  if (dst_n == SFH_SIZE_FROM_TRAILER || !d_index || ((uintptr_t)d_index & 7) || nseg != (size_t)chunks_of((size_t)dst_n) ||
      nseg > ((size_t)1 << 31) - 1)
    return fail(ctx, SFH_E_INVALID_ARG, "index: 8-byte aligned, nseg = max(1, ceil(dst_n / 32768))", hipSuccess);
  if (int rc = check_any_waves(ctx, src_n)) return rc;
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  const uint64_t n = src_n;
  AnyBatch R;
  if (int rc = any_batch_recover(ctx, 1, &d_src, &n, container, nullptr, &dst_n, d_index, s, R)) return rc;
  if (R.st[0])
    return fail(ctx, SFH_E_NOT_INDEXABLE, R.st[0] == SFH_ITEM_NOT_INDEXABLE ? "not block-flushed every 32 KiB" : "the wrapper header does not parse",
                hipSuccess);
  return d_depends ? any_batch_decode(ctx, 1, &d_src, &n, container, nullptr, d_index, s, R, d_depends) : SFH_OK;
}

int sfh_recover_index(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, uint64_t dst_n, uint64_t* index, size_t nseg,
                      uint8_t* depends) {
  if (int rc = check_any(ctx, src, src_n, container, dst_n, false)) return rc;
  if (!index || dst_n == SFH_SIZE_FROM_TRAILER || nseg != (size_t)chunks_of((size_t)dst_n))
    return fail(ctx, SFH_E_INVALID_ARG, "index, nseg = max(1, ceil(dst_n / 32768))", hipSuccess);
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = ctx->d_anyix.grow(ctx, nseg + 1, "recovered index");
  if (!rc) rc = host_up(ctx, src, src_n, depends ? nseg : 0);  // (the flags come down through d_out)
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  if ((rc = sfh_recover_index_device(ctx, ctx->d_in, src_n, container, dst_n, ctx->d_anyix, nseg, depends ? ctx->d_out : nullptr, s)))
    return rc;
  SF_HIP(hipMemcpyAsync(index, ctx->d_anyix, (nseg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s), "D2H index");
  if (depends) SF_HIP(hipMemcpyAsync(depends, ctx->d_out, nseg, hipMemcpyDeviceToHost, s), "D2H depends");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

int sfh_decompress_any_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, void* d_dst, uint64_t dst_n,
                              uint32_t* status, void* stream) {
  if (int rc = check_any(ctx, d_src, src_n, container, dst_n, true)) return rc;
  if (!status || (!d_dst && dst_n) || ((uintptr_t)d_dst & 15))
    return fail(ctx, SFH_E_INVALID_ARG, "argument (status, dst 16-byte aligned)", hipSuccess);
  if (int rc = check_any_waves(ctx, src_n)) return rc;
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  // The call takes no capacity: the size asked for is the capacity, and no ISIZE is above the one of a size from the trailer.
  const uint64_t n = src_n, cap = dst_n == SFH_SIZE_FROM_TRAILER ? UINT64_MAX : dst_n;
  AnyBatch R;
  if (int rc = any_batch_recover(ctx, 1, &d_src, &n, container, &cap, &dst_n, nullptr, s, R)) return rc;
  if (R.st[0] == SFH_ITEM_NOT_INDEXABLE) return fail(ctx, SFH_E_NOT_INDEXABLE, "not block-flushed every 32 KiB", hipSuccess);
  if (R.st[0]) {  // container.hpp's answer for the wrapper (SrcTooSmall, Error, DstTooSmall)
    *status = R.st[0];
    return SFH_OK;
  }
  if (int rc = any_batch_decode(ctx, 1, &d_src, &n, container, &d_dst, ctx->d_anyix, s, R)) return rc;
  *status = R.st[0];
  if (R.st[0]) snprintf(ctx->err, sizeof ctx->err, "DecompressStatus %u", R.st[0]);
  return SFH_OK;
}

int sfh_decompress_any(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, void* dst, uint64_t dst_cap,
                       uint64_t dst_n, uint64_t* dst_n_out, uint32_t* status) {
  if (int rc = check_any(ctx, src, src_n, container, dst_n, false)) return rc;
  if (!status || (!dst && dst_cap)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  const uint64_t out_n = dst_n == SFH_SIZE_FROM_TRAILER ? trailer_isize(src, src_n) : dst_n;
  if (out_n > dst_cap) return fail(ctx, SFH_E_DST_TOO_SMALL, "dst_cap below the output size", hipSuccess);
  if (dst_n_out) *dst_n_out = out_n;
  int rc = host_up(ctx, src, src_n, out_n);
  if (!rc) rc = sfh_decompress_any_device(ctx, ctx->d_in, src_n, container, ctx->d_out, out_n, status, ctx->stream);
  if (rc) return rc;
  return *status ? SFH_OK : host_down(ctx, dst, out_n);
}

int sfh_recover_index_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                                   const uint64_t* dst_n, uint64_t* d_index, uint32_t* status, void* stream) {
  int rc = check_any_batch(ctx, count, d_srcs, src_n, container, nullptr, nullptr, dst_n, d_index, true, status, true);
  if (rc || count == 0) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s))) return rc;
  AnyBatch R;
  if ((rc = any_batch_recover(ctx, count, d_srcs, src_n, container, nullptr, dst_n, d_index, s, R))) return rc;
  for (size_t i = 0; i < count; ++i) status[i] = R.st[i] ? SFH_ITEM_NOT_INDEXABLE : 0u;  // (a wrapper that does not parse too)
  return SFH_OK;
}

int sfh_decompress_any_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                                    void* const* d_dsts, const uint64_t* dst_cap, const uint64_t* dst_n, uint64_t* dst_n_out,
                                    uint32_t* status, void* stream) {
  int rc = check_any_batch(ctx, count, d_srcs, src_n, container, d_dsts, dst_cap, dst_n, nullptr, false, status, true);
  if (rc || count == 0) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s))) return rc;
  AnyBatch R;
  if ((rc = any_batch_recover(ctx, count, d_srcs, src_n, container, dst_cap, dst_n, nullptr, s, R))) return rc;
  if ((rc = any_batch_decode(ctx, count, d_srcs, src_n, container, d_dsts, ctx->d_anyix, s, R))) return rc;
  for (size_t i = 0; i < count; ++i) {
    status[i] = R.st[i];
    if (dst_n_out) dst_n_out[i] = R.out_n[i];
  }
  return SFH_OK;
}

int sfh_recover_index_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                            const uint64_t* dst_n, uint64_t* index, uint32_t* status) {
  int rc = check_any_batch(ctx, count, srcs, src_n, container, nullptr, nullptr, dst_n, index, true, status, false);
  if (rc || count == 0) return rc;
  size_t entries = count;
  for (size_t i = 0; i < count; ++i) entries += chunks_of((size_t)dst_n[i]);
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, nullptr))) return rc;  // (no output staging: the index comes down by itself)
  if ((rc = ctx->d_index.grow(ctx, entries, "index staging"))) return rc;
  AnyBatch R;
  if ((rc = any_batch_recover(ctx, count, B.d_srcs.data(), src_n, container, nullptr, dst_n, ctx->d_index, s, R))) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  SF_HIP(hipMemcpyAsync(index, ctx->d_index, entries * sizeof(uint64_t), hipMemcpyDeviceToHost, s), "D2H index");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  for (size_t i = 0; i < count; ++i) status[i] = R.st[i] ? SFH_ITEM_NOT_INDEXABLE : 0u;  // (a wrapper that does not parse too)
  return SFH_OK;
}

int sfh_decompress_any_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                             void* const* dsts, const uint64_t* dst_cap, const uint64_t* dst_n, uint64_t* dst_n_out,
                             uint32_t* status) {
  int rc = check_any_batch(ctx, count, srcs, src_n, container, dsts, dst_cap, dst_n, nullptr, false, status, false);
  if (rc || count == 0) return rc;
  // An item's slot is its output size (ISIZE is read here); one whose size is above its capacity gets no slot, and the device
  // call reports it.
  std::vector<uint64_t> slot;
  try {
    slot.resize(count);
  } catch (...) {
    return fail(ctx, SFH_E_NOMEM, "host memory", hipSuccess);
  }
  for (size_t i = 0; i < count; ++i) {
    const uint64_t n = dst_n[i] == SFH_SIZE_FROM_TRAILER ? trailer_isize(srcs[i], src_n[i]) : dst_n[i];
    slot[i] = n <= dst_cap[i] ? n : 0;
  }
  Staged B;
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, slot.data()))) return rc;
  AnyBatch R;
  rc = any_batch_recover(ctx, count, B.d_srcs.data(), src_n, container, slot.data(), dst_n, nullptr, s, R);
  if (!rc) rc = any_batch_decode(ctx, count, B.d_srcs.data(), src_n, container, B.d_dsts.data(), ctx->d_anyix, s, R);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  for (size_t i = 0; i < count; ++i) {
    status[i] = R.st[i];
    if (dst_n_out) dst_n_out[i] = R.out_n[i];
  }
  return staged_down(ctx, B, count, dsts, R.out_n.data(), status);
}

int sfh_last_recover_stats(sfh_ctx* ctx, float ms[2], uint64_t counts[2]) {
  if (!ctx || !ms || !counts) return SFH_E_INVALID_ARG;
  ms[0] = ctx->any_ms[0];
  ms[1] = ctx->any_ms[1];
  counts[0] = ctx->any_counts[0];
  counts[1] = ctx->any_counts[1];
  return SFH_OK;
}

int sfh_inflate_stream_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, void* d_dst, uint64_t dst_cap,
                              uint64_t* dst_n_out, uint32_t* status, void* stream) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if ((!d_src && src_n) || !stream_container(container) || !dst_n_out || !status || (!d_dst && dst_cap))
    return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 15))
    return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 4, dst 16)", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  return stream_one(ctx, d_src, src_n, container, d_dst, dst_cap, false, dst_n_out, status, s);
}

int sfh_inflate_stream(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, void* dst, uint64_t dst_cap,
                       uint64_t* dst_n_out, uint32_t* status) {
  if (!ctx) return SFH_E_INVALID_ARG;
  if ((!src && src_n) || !stream_container(container) || !dst_n_out || !status || (!dst && dst_cap))
    return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  int rc = host_up(ctx, src, src_n, 0);  // (the driver sizes d_out once it knows the output's)
  if (!rc) rc = stream_one(ctx, ctx->d_in, src_n, container, dst, dst_cap, dst != nullptr, dst_n_out, status, ctx->stream);
  if (rc) return rc;
  return (dst && *status == 0) ? host_down(ctx, dst, *dst_n_out) : SFH_OK;  // (staged: the one item lies at ctx->d_out)
}

int sfh_inflate_stream_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                    uint32_t container, void* const* d_dsts, const uint64_t* dst_cap, uint64_t* dst_n_out,
                                    uint32_t* status, void* stream) {
  int rc = check_stream_batch(ctx, count, d_srcs, src_n, container, d_dsts, dst_cap, dst_n_out, status, true);
  if (rc || count == 0) return rc;
  hipStream_t s;
  if ((rc = begin_call(ctx, stream, &s))) return rc;
  return stream_batch_run(ctx, count, d_srcs, src_n, container, d_dsts, dst_cap, false, nullptr, dst_n_out, status, s);
}

int sfh_inflate_stream_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                             void* const* dsts, const uint64_t* dst_cap, uint64_t* dst_n_out, uint32_t* status) {
  int rc = check_stream_batch(ctx, count, srcs, src_n, container, dsts, dst_cap, dst_n_out, status, false);
  if (rc || count == 0) return rc;
  Staged B;  // (the output: packed by its size in ctx->d_out, laid out by the driver once the sizes are known)
  hipStream_t s = ctx->stream;
  if ((rc = staged_up(ctx, B, count, srcs, src_n, nullptr))) return rc;
  if ((rc = stream_batch_run(ctx, count, B.d_srcs.data(), src_n, container, dsts, dst_cap, true, &B.out_off, dst_n_out, status, s))) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  return dsts ? staged_down(ctx, B, count, dsts, dst_n_out, status) : SFH_OK;  // (no dsts: a size query)
}

int sfh_last_stream_stats(sfh_ctx* ctx, float ms[SFH_STREAM_NSTAGES], uint64_t counts[SFH_STREAM_NCOUNTS]) {
  if (!ctx || !ms || !counts) return SFH_E_INVALID_ARG;
  for (int k = 0; k < SFH_STREAM_NSTAGES; ++k) ms[k] = ctx->stm_ms[k];
  for (int k = 0; k < SFH_STREAM_NCOUNTS; ++k) counts[k] = ctx->stm_counts[k];
  return SFH_OK;
}

size_t sfh_last_decode_scratch_bytes(const sfh_ctx* ctx) { return ctx ? ctx->last_dtok_bytes : 0; }

int sfh_last_inflate_ms(sfh_ctx* ctx, float ms[SFH_INFLATE_NSTAGES]) {
  if (!ctx || !ms || !ctx->ev_inf_valid) return SFH_E_INVALID_ARG;
  for (int k = 0; k < SFH_INFLATE_NSTAGES; ++k) ms[k] = 0.f;
  for (uint32_t b = 0; b < ctx->ev_inf_batches; ++b)  // a stage's time over every batch of the call
    for (int k = 0; k < SFH_INFLATE_NSTAGES; ++k) {
      float t = 0.f;
      const Event* ev = &ctx->ev_inf[(size_t)b * (SFH_INFLATE_NSTAGES + 1)];
      SF_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]), "elapsed");
      ms[k] += t;
    }
  return SFH_OK;
}

const char* sfh_inflate_stage_name(int stage) {
  static const char* names[SFH_INFLATE_NSTAGES] = {"k_inflate_tokens", "k_inflate_bytes"};
  return (stage >= 0 && stage < SFH_INFLATE_NSTAGES) ? names[stage] : "";
}

int sfh_checksum_device(sfh_ctx* ctx, const void* d_src, size_t n, uint32_t kind, uint32_t* out, void* stream) {
  if (!ctx || (!d_src && n) || !out || (kind != SFH_ZLIB && kind != SFH_GZIP)) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  if ((uintptr_t)d_src & 15) return fail(ctx, SFH_E_INVALID_ARG, "device pointer alignment (src 16)", hipSuccess);
  if (n > ((size_t)1 << 44)) return fail(ctx, SFH_E_INVALID_ARG, "input too large", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  const uint32_t nchunks = chunks_of(n);
  int rc = ensure_sums(ctx, nchunks);
  if (!rc) rc = order_behind_last_call(ctx, s);
  if (rc) return rc;
  SF_HIP(sf::launch_checksum((const uint8_t*)d_src, n, nchunks, kind, ctx->ws.sums, s), "launch k_checksum");
  SF_HIP(sf::launch_wrap(ctx->ws.sums, nchunks, n, kind, nullptr, nullptr, ctx->d_value, s), "launch k_wrap");
  SF_HIP(hipMemcpyAsync(out, ctx->d_value, sizeof *out, hipMemcpyDeviceToHost, s), "copy checksum");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  return SFH_OK;
}

uint32_t sfh_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return sf::crc32_combine(crc_a, crc_b, len_b); }
uint32_t sfh_adler32_combine(uint32_t adler_a, uint32_t adler_b, uint64_t len_b) {
  return sf::adler32_combine(adler_a, adler_b, len_b);
}

int sfh_compress_multi(sfh_ctx* const* ctxs, int nctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n,
                       const sfh_options* opt) {
  if (!ctxs || nctx <= 0 || (!src && n) || !dst || !out_n || check_opt(opt)) return SFH_E_INVALID_ARG;
  for (int i = 0; i < nctx; ++i) {
    if (!ctxs[i]) return SFH_E_INVALID_ARG;
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return fail(ctxs[i], SFH_E_INVALID_ARG, "sfh_compress_multi: the same ctx twice", hipSuccess);
  }
  if (cap < sfh_compress_bound(n, 0)) return fail(ctxs[0], SFH_E_DST_TOO_SMALL, "cap < sfh_compress_bound(n)", hipSuccess);
  sfh_options o;
  if (opt) o = *opt; else sfh_default_options(&o);
  // the strip size is fixed once, from the whole input: every shard is a whole number of strips, so the
  // shards' streams are exactly the pieces of the single-call stream
  o.block_bytes = resolve_block_bytes(o.block_bytes, n, o.effort);
  // shards: equal numbers of strips, the tail shards may be empty (they then contribute nothing)
  const size_t cps = o.block_bytes / sf::kChunk;  // chunks per strip
  const size_t nstrips = n ? (n + o.block_bytes - 1) / o.block_bytes : 1;
  const size_t per = ((nstrips + (size_t)nctx - 1) / (size_t)nctx) * cps;
  struct Shard {
    size_t lo = 0, len = 0, bound_off = 0, out = 0;
    uint32_t sum = 0;
    int rc = SFH_OK;
    bool used = false;
  };
  std::vector<Shard> sh((size_t)nctx);
  int last = 0;
  const size_t hdr = sf::wrapper_header_bytes(o.container);
  size_t off = hdr;  // the wrapper header goes in front of the first slice
  for (int i = 0; i < nctx; ++i) {
    Shard& s = sh[(size_t)i];
    s.lo = std::min(n, (size_t)i * per * sf::kChunk);
    const size_t hi = std::min(n, ((size_t)i + 1) * per * sf::kChunk);
    s.len = hi - s.lo;
    s.used = s.len > 0 || i == 0;  // an empty input is one empty stream on the first ctx
    if (s.used) last = i;
    s.bound_off = off;
    if (s.used) off += sfh_compress_bound(s.len, 0);
  }
  // every shard compresses into its own slice of dst (sized by the bound), then the slices are closed up
  std::vector<std::thread> workers;
  for (int i = 0; i < nctx; ++i) {
    if (!sh[(size_t)i].used) continue;
    workers.emplace_back([&, i] {
      Shard& s = sh[(size_t)i];
      sfh_options so = o;
      so.container = SFH_RAW;
      so.final_stream = (i == last) ? o.final_stream : 0u;
      // a stream is shorter than its bound by more than the wrapper (>= 345 bytes of slack per chunk), so the
      // slices, laid out bound after bound behind the header, stay inside cap = sfh_compress_bound(n)
      s.rc = sfh_compress(ctxs[i], (const uint8_t*)src + s.lo, s.len, (uint8_t*)dst + s.bound_off,
                          sfh_compress_bound(s.len, 0), &s.out, &so);
      if (s.rc == SFH_OK && o.container)  // the shard is still staged on the device: checksum it there
        s.rc = sfh_checksum_device(ctxs[i], ctxs[i]->d_in, s.len, o.container, &s.sum, nullptr);
    });
  }
  for (auto& w : workers) w.join();
  for (int i = 0; i < nctx; ++i)
    if (sh[(size_t)i].used && sh[(size_t)i].rc != SFH_OK) return sh[(size_t)i].rc;
  uint8_t* d = (uint8_t*)dst;
  size_t pos = hdr;
  uint32_t sum = 0;
  bool first = true;
  for (int i = 0; i < nctx; ++i) {
    const Shard& s = sh[(size_t)i];
    if (!s.used) continue;
    memmove(d + pos, d + s.bound_off, s.out);  // pos <= bound_off: slices only move down
    pos += s.out;
    if (o.container) {
      sum = first ? s.sum : (o.container == SFH_ZLIB ? sf::adler32_combine(sum, s.sum, s.len) : sf::crc32_combine(sum, s.sum, s.len));
      first = false;
    }
  }
  if (o.container == SFH_ZLIB) {
    d[0] = 0x78;
    d[1] = 0x9C;
    for (int k = 0; k < 4; ++k) d[pos + (size_t)k] = (uint8_t)(sum >> (24 - 8 * k));
    pos += 4;
  } else if (o.container == SFH_GZIP) {
    static const uint8_t h[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
    memcpy(d, h, 10);
    const uint32_t isize = (uint32_t)n;
    for (int k = 0; k < 4; ++k) {
      d[pos + (size_t)k] = (uint8_t)(sum >> (8 * k));
      d[pos + 4 + (size_t)k] = (uint8_t)(isize >> (8 * k));
    }
    pos += 8;
  }
  *out_n = pos;
  return SFH_OK;
}

// ---- one process per GPU: concatenation over RCCL (binding: struct Rccl above) ----
int sfh_gather_offsets(const uint64_t* sizes, int nranks, uint64_t base, uint64_t cap, uint64_t* offsets) {
  if (!sizes || !offsets || nranks <= 0) return SFH_E_INVALID_ARG;
  uint64_t at = base;
  for (int r = 0; r < nranks; ++r) {
    offsets[r] = at;
    if (sizes[r] > UINT64_MAX - at) return SFH_E_INVALID_ARG;
    at += sizes[r];
  }
  offsets[nranks] = at;
  return at > cap ? SFH_E_DST_TOO_SMALL : SFH_OK;
}

int sfh_comm_ranks(void* nccl_comm, int* nranks, int* rank) {
  if (!nccl_comm || !nranks || !rank) return SFH_E_INVALID_ARG;
  const Rccl& R = rccl();
  if (!R.ok || R.CommCount(nccl_comm, nranks) != 0 || R.CommUserRank(nccl_comm, rank) != 0) return SFH_E_COMM;
  return SFH_OK;
}

int sfh_gather_streams(sfh_ctx* ctx, void* nccl_comm, int root, const void* d_stream, const uint64_t* d_size, void* d_out,
                       uint64_t base, uint64_t cap, uint64_t* h_sizes, uint64_t* out_end, void* stream) {
  if (!ctx || !nccl_comm || !d_stream || !d_size || !h_sizes || !out_end) return fail(ctx, SFH_E_INVALID_ARG, "argument", hipSuccess);
  const Rccl& R = rccl();
  if (!R.ok) {
    snprintf(ctx->err, sizeof ctx->err, "%s", R.why);
    return SFH_E_COMM;
  }
  int nranks = 0, rank = -1, rc;
  if ((rc = R.CommCount(nccl_comm, &nranks)) != 0) return comm_fail(ctx, "ncclCommCount", rc);
  if ((rc = R.CommUserRank(nccl_comm, &rank)) != 0) return comm_fail(ctx, "ncclCommUserRank", rc);
  if (root < 0 || root >= nranks || (rank == root && !d_out)) return fail(ctx, SFH_E_INVALID_ARG, "root / d_out", hipSuccess);
  hipStream_t s;
  if (int rc = begin_call(ctx, stream, &s)) return rc;
  // Every rank contributes {size, base, cap, its d_stream, its d_out}: sizes are what is gathered; base and cap must be the
  // same on all ranks, and the root's two addresses let EVERY rank judge the root's own placement -- so every rank reaches
  // the same verdict BEFORE any transfer is posted, and nobody is left waiting in a send whose receive was refused.
  constexpr int kRec = 5;
  if (ctx->sizes.grow(ctx, ((size_t)nranks + 1) * kRec, "sizes")) return SFH_E_HIP;  // (this call's code for it, as before)
  uint64_t* const d_mine = ctx->sizes.d + (size_t)nranks * kRec;  // this rank's record, behind the gathered ones
  uint64_t* const h_mine = ctx->sizes.h + (size_t)nranks * kRec;
  h_mine[1] = base;
  h_mine[2] = cap;
  h_mine[3] = (uint64_t)(uintptr_t)d_stream;
  h_mine[4] = (uint64_t)(uintptr_t)d_out;
  // the compressor may have run on another stream of this ctx: its size word is final behind ev_done
  rc = order_behind_last_call(ctx, s);
  if (rc) return rc;
  SF_HIP(hipMemcpyAsync(d_mine + 1, h_mine + 1, (kRec - 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s), "record");
  SF_HIP(hipMemcpyAsync(d_mine, d_size, sizeof(uint64_t), hipMemcpyDeviceToDevice, s), "size word");
  if ((rc = R.AllGather(d_mine, ctx->sizes.d, kRec, kNcclUint64, nccl_comm, s)) != 0) return comm_fail(ctx, "ncclAllGather", rc);
  SF_HIP(hipMemcpyAsync(ctx->sizes.h, ctx->sizes.d, (size_t)nranks * kRec * sizeof(uint64_t), hipMemcpyDeviceToHost, s), "sizes read-back");
  SF_HIP(hipStreamSynchronize(s), "stream sync");
  // (no exception may cross the C boundary: the offsets live in a nothrow allocation)
  struct Free { void operator()(uint64_t* p) const { free(p); } };
  const std::unique_ptr<uint64_t, Free> off_mem((uint64_t*)malloc(((size_t)nranks + 1) * sizeof(uint64_t)));
  if (!off_mem) return fail(ctx, SFH_E_NOMEM, "sfh_gather_streams: offsets", hipSuccess);
  uint64_t* const off = off_mem.get();
  bool agree = true;
  for (int r = 0; r < nranks; ++r) {
    const uint64_t* rec = ctx->sizes.h + (size_t)r * kRec;
    h_sizes[r] = rec[0];
    agree = agree && rec[1] == base && rec[2] == cap;
  }
  if (!agree) return fail(ctx, SFH_E_INVALID_ARG, "sfh_gather_streams: the ranks disagree on base / cap", hipSuccess);  // (on every rank alike)
  rc = sfh_gather_offsets(h_sizes, nranks, base, cap, off);
  *out_end = off[(size_t)nranks];
  if (rc != SFH_OK) return fail(ctx, rc, "sfh_gather_streams: the gathered streams do not fit cap", hipSuccess);
  {
    // the root's own stream: already at its place in d_out, or clear of everything the gather writes -- anything between
    // would be overwritten by a peer's bytes or copied onto itself
    const uint64_t* rr = ctx->sizes.h + (size_t)root * kRec;
    const uint64_t rs = rr[3], ro = rr[4], rn = rr[0];
    const uint64_t w0 = ro + base, w1 = ro + off[(size_t)nranks];
    if (rn && rs != ro + off[(size_t)root] && rs < w1 && rs + rn > w0)
      return fail(ctx, SFH_E_INVALID_ARG, "sfh_gather_streams: the root's d_stream overlaps the gathered range of d_out without being at its own place", hipSuccess);
  }
  if (rank != root) {
    if (h_sizes[rank] && (rc = R.Send(d_stream, (size_t)h_sizes[rank], kNcclUint8, root, nccl_comm, s)) != 0) return comm_fail(ctx, "ncclSend", rc);
    return SFH_OK;
  }
  uint8_t* out = (uint8_t*)d_out;
  if ((rc = R.GroupStart()) != 0) return comm_fail(ctx, "ncclGroupStart", rc);
  for (int r = 0; r < nranks; ++r) {
    if (r == root || !h_sizes[r]) continue;
    if ((rc = R.Recv(out + off[(size_t)r], (size_t)h_sizes[r], kNcclUint8, r, nccl_comm, s)) != 0) {
      (void)R.GroupEnd();
      return comm_fail(ctx, "ncclRecv", rc);
    }
  }
  if ((rc = R.GroupEnd()) != 0) return comm_fail(ctx, "ncclGroupEnd", rc);
  if (h_sizes[root] && (const uint8_t*)d_stream != out + off[(size_t)root])
    SF_HIP(hipMemcpyAsync(out + off[(size_t)root], d_stream, (size_t)h_sizes[root], hipMemcpyDeviceToDevice, s), "own stream");
  return SFH_OK;
}

void sfh_set_profiling(sfh_ctx* ctx, int on) {
  if (ctx) ctx->profiling = on;
}

int sfh_last_stage_ms(sfh_ctx* ctx, float ms[SFH_NSTAGES]) {
  if (!ctx || !ms || !ctx->ev_valid) return SFH_E_INVALID_ARG;
  // summed over every batch of the call (a > 1 GiB device call or any host-buffer call runs several)
  for (int k = 0; k < SFH_NSTAGES; ++k) ms[k] = 0.f;
  for (uint32_t b = 0; b < ctx->ev_batches; ++b) {
    const Event* e = &ctx->ev[(size_t)b * sfh_ctx::kEvPerBatch];
    for (int k = 0; k < 4; ++k) {
      float t = 0.f;
      SF_HIP(hipEventElapsedTime(&t, e[k], e[k + 1]), "elapsed");
      ms[k] += t;
    }
  }
  const size_t last = (size_t)ctx->ev_batches * sfh_ctx::kEvPerBatch;
  SF_HIP(hipEventElapsedTime(&ms[4], ctx->ev[last - 1], ctx->ev[last]), "elapsed");  // k_checksum + k_wrap
  return SFH_OK;
}

const char* sfh_stage_name(int stage) {
  static const char* names[SFH_NSTAGES] = {"k_lz77", "k_plan", "k_scan", "k_emit", "k_checksum"};
  return (stage >= 0 && stage < SFH_NSTAGES) ? names[stage] : "";
}

int sfh_debug_read(sfh_ctx* ctx, int what, void* host_dst, size_t bytes) {
  if (ctx && host_dst && what == SFH_DBG_STREAM_MEMBERS) {  // host memory, whatever the last compress call was
    if (!ctx->stm_members_valid || bytes < 8) return SFH_E_INVALID_ARG;
    const uint64_t count = ctx->stm_members.size();
    memcpy(host_dst, &count, 8);
    const size_t fit = std::min<size_t>(count, (bytes - 8) / sizeof(sf::StreamMember));
    if (fit) memcpy(static_cast<uint8_t*>(host_dst) + 8, ctx->stm_members.data(), fit * sizeof(sf::StreamMember));
    return SFH_OK;
  }
  if (!ctx || !host_dst || !ctx->last_chunks) return SFH_E_INVALID_ARG;
  // per-batch arrays hold the last batch of the call (all of it for up to kBatchChunks chunks); each array is read no
  // further than it was allocated: the last call may be a decode on a context whose compressor arrays are smaller or absent
  const size_t nlast = std::min<size_t>(ctx->last_chunks, std::max<uint32_t>(ctx->batch_chunks, sf::kMaxStrip / sf::kChunk));
  const size_t nc = std::min<size_t>(nlast, ctx->cap_batch), nidx = std::min<size_t>(ctx->last_chunks, ctx->cap_chunks);
  if (int rc = wait_idle(ctx)) return rc;  // whatever stream the last call ran on
  const void* p = nullptr;
  size_t avail = 0;
  switch (what) {
    case SFH_DBG_NTOK: p = ctx->ws.ntok; avail = nc * 4; break;
    case SFH_DBG_TOKENS: p = ctx->ws.tokens; avail = ctx->cap_dtok >= nlast ? nlast * sf::kChunk * 4 : 0; break;
    case SFH_DBG_ITEMS: p = ctx->ws.items; avail = nc * sf::kChunk * 2; break;
    case SFH_DBG_NITEMS: p = ctx->ws.nitems; avail = nc * 4; break;
    case SFH_DBG_RITEM: {  // the high halves of the region words
      if (!ctx->ws.rtok || bytes % 4 || bytes > nc * sf::kSubRegions * 4) return SFH_E_INVALID_ARG;
      SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
      SF_HIP(hipMemcpy(host_dst, ctx->ws.rtok, bytes, hipMemcpyDeviceToHost), "debug copy");
      for (size_t k = 0; k < bytes / 4; ++k) static_cast<uint32_t*>(host_dst)[k] >>= 16;
      return SFH_OK;
    }
    case SFH_DBG_HIST: p = ctx->ws.hist; avail = nc * sf::kHistStride * 4; break;
    case SFH_DBG_PLAN: p = ctx->ws.plan; avail = nc * sizeof(sf::ChunkPlan); break;
    case SFH_DBG_OFFSETS: p = ctx->ws.offsets; avail = nidx * 8; break;
    case SFH_DBG_SUBINDEX: p = ctx->ws.subidx; avail = nidx * SFH_SUBINDEX_WORDS * 4; break;
    case SFH_DBG_STAMPS: p = ctx->ws.stamps; avail = p ? nc * 128 : 0; break;
    case SFH_DBG_SEGINFO: p = ctx->ws.seginfo; avail = std::min<size_t>(ctx->last_chunks * sizeof(sf::SegInfo), ctx->seginfo_cap); break;
    case SFH_DBG_LENS: {
      if (!ctx->ws.codes || bytes > nc * 320) return SFH_E_INVALID_ARG;
      SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
      SF_HIP(hipMemcpy2D(host_dst, 320, (const uint8_t*)ctx->ws.codes + offsetof(sf::ChunkCodes, lens),
                         sizeof(sf::ChunkCodes), 320, bytes / 320, hipMemcpyDeviceToHost), "debug copy");
      return SFH_OK;
    }
    default: return SFH_E_INVALID_ARG;
  }
  if (!p || bytes > avail) return SFH_E_INVALID_ARG;
  SF_HIP(hipSetDevice(ctx->device), "hipSetDevice");
  SF_HIP(hipMemcpy(host_dst, p, bytes, hipMemcpyDeviceToHost), "debug copy");
  return SFH_OK;
}

}  // extern "C"
