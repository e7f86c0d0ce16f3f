/*
 * starflate_hip.h -- C-ABI of the MI355X DEFLATE compressor (libstarflate_hip.so).
 *
 * The reference (garymm/starflate) has no FFI/plugin interface and no
 * compressor (README.md:5-7).  The boundary kept here is the shape of its one
 * public function,
 *     starflate::decompress(span<const byte> src, span<byte> dst) -> DecompressStatus
 *     (/root/reference/src/decompress.hpp:63-71):
 * caller-owned buffers in, callee never allocates output, no exceptions, a small
 * integer status out.  By default sfh_compress* produce raw RFC 1951 streams (no
 * zlib/gzip wrapper, as /root/reference/tools/deflate_compress.py:8-13 does for the
 * reference's fixtures) that the reference's decompress() inverts; the wrappers
 * that tool strips (RFC 1950 / RFC 1952) are available through sfh_options.container.
 * The C++23 wrapper starflate::compress() (include/starflate/compress.hpp) is the
 * only intended caller besides tests and bench.py (ctypes).
 *
 * Threading: a ctx is not thread-safe; distinct ctxs are independent.  A ctx owns
 * its device scratch; all other buffers are caller-owned.
 */
#ifndef STARFLATE_HIP_H
#define STARFLATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfh_ctx sfh_ctx;

/* negative return values of every sfh_* function returning int */
enum sfh_status {
  SFH_OK = 0,
  SFH_E_INVALID_ARG = -1,   /* null pointer, bad option value, misaligned device pointer */
  SFH_E_DST_TOO_SMALL = -2, /* cap < sfh_compress_bound(n) -- mirrors DecompressStatus::DstTooSmall */
  SFH_E_NO_DEVICE = -3,     /* no HIP device / device index out of range */
  SFH_E_HIP = -4,           /* a HIP runtime call failed; see sfh_last_error() */
  SFH_E_NOMEM = -5,         /* device scratch allocation failed */
  SFH_E_COMM = -6,          /* RCCL not loadable, or an RCCL call failed; see sfh_last_error() */
  SFH_E_UNSUPPORTED = -7,   /* the effort asked for rests on LDS behaviour this device does not show (sfh_lds_order_check) */
  SFH_E_NOT_INDEXABLE = -8  /* sfh_recover_index* / sfh_decompress_any*: the stream is not block-flushed every 32 KiB of
                               output (the walk of DESIGN.md 3a ends before it found every segment); nothing was decoded.
                               sfh_dz_read_index* / sfh_decompress_dz*: the gzip header carries no dictzip table of 32 KiB chunks.
                               sfh_decompress_bgzf_device: a member of the BGZF file holds more than 32768 bytes (ISIZE), so it
                               is no narrow row of the indexed decoder; nothing was decoded (sfh_decompress_bgzf_wide_device
                               and sfh_decompress_bgzf read such files).  sfh_decompress_bgzf_wide_device: a member claims more
                               than 65536 bytes, which is not BGZF */
};

/* block strategy (inverse of src/decompress.cpp:416-458 dispatch) */
enum sfh_strategy {
  SFH_AUTO = 0,   /* per chunk: smallest of stored / fixed / dynamic */
  SFH_STORED = 1, /* BTYPE 00 only  (src/decompress.cpp:416-436) */
  SFH_FIXED = 2,  /* BTYPE 01 only  (src/decompress.cpp:437-446) */
  SFH_DYNAMIC = 3 /* BTYPE 10 only  (src/decompress.cpp:447-458) */
};

/* stream wrapper around the raw DEFLATE data (what tools/deflate_compress.py:8-13 removes) */
enum sfh_container {
  SFH_RAW = 0,  /* RFC 1951 only: what the reference's decompress() reads */
  SFH_ZLIB = 1, /* RFC 1950: 78 9C, stream, Adler-32 big-endian */
  SFH_GZIP = 2, /* RFC 1952: 1F 8B 08 00, MTIME 0, XFL 0, OS 255, stream, CRC-32, ISIZE (both little-endian) */
  SFH_DICTZIP = 3, /* SFH_GZIP at block_bytes = 32768 whose header carries dictzip(1)'s random-access table (FLG = FEXTRA, an
                     'RA' subfield: VER 1, CHLEN 32768, CHCNT, the compressed bytes of every 32 KiB chunk; "Seekable gzip" below).
                     In sfh_options.container of sfh_compress, sfh_compress_device and sfh_compress_device_async ONLY: the
                     batched calls, sfh_compress_multi and the gathered multi-process path refuse it (SFH_E_INVALID_ARG; out of
                     scope so far), and so does every decoder's `container` argument -- to a decoder such a file is an SFH_GZIP
                     stream (FEXTRA is skipped); sfh_dz_read_index* / sfh_decompress_dz* read the table */
  SFH_GZIP_MEMBERS = 4 /* a file of gzip members (RFC 1952 2.2), zero bytes allowed behind each: `cat a.gz b.gz`, the joined items
                          of sfh_compress_batch(SFH_GZIP), WARC files, BGZF without its 'BC' field.  Taken by sfh_inflate_stream,
                          sfh_inflate_stream_device, sfh_inflate_stream_batch and sfh_inflate_stream_batch_device ONLY ("Files of
                          gzip members" below); every other decoder and every compress call refuses it (SFH_E_INVALID_ARG, before
                          anything is enqueued), and sfh_compress_bound_container answers 0 */
};

typedef struct sfh_options {
  uint32_t strategy;     /* enum sfh_strategy */
  uint32_t final_stream; /* 1: last block carries BFINAL (src/decompress.cpp:410-415);
                            0: stream ends byte-aligned and non-final (a GPU shard
                            that is not the last one) */
  uint32_t lazy;         /* 0..3: lazy match deferral, positions of look-ahead (default 3) */
  uint32_t no_stored_fast_path; /* 0 (default): a 32 KiB chunk whose first 8 KiB parse to (almost) only
                            literals is not searched further and is coded as literals throughout (high-entropy
                            data -> stored blocks); the chunk behind it in its strip is probed on its first
                            2 KiB only (a sixteenth of the match work while the data stays like that); with
                            SFH_STRATEGY_AUTO a full chunk whose first 8 KiB of BYTES are as good as uniform (their
                            entropy within 64 bytes of 8 KiB) is stored outright, its other 24 KiB never fetched by the
                            match kernel (round 6);
                            1: always search the whole chunk */
  uint32_t container;    /* enum sfh_container; SFH_ZLIB / SFH_GZIP / SFH_DICTZIP need final_stream = 1.  The checksum is
                            computed on the GPU from the same device buffer (two more launches).  SFH_DICTZIP: block_bytes
                            must be 0 or 32768 (0 is 32768 then, whatever n is: the table promises independent chunks) and
                            n <= SFH_DZ_MAX_CHUNKS * 32768, else SFH_E_INVALID_ARG before anything is enqueued */
  uint32_t block_bytes;  /* bytes of input coded independently of what precedes them (a "strip"): a multiple of
                            32768 up to 16 MiB; 0 (default) = SFH_DEFAULT_BLOCK_BYTES, more (SFH_LARGE_BLOCK_BYTES,
                            SFH_CHAIN_BLOCK_BYTES with the chain efforts) for inputs of half a GiB and up, less for inputs
                            too small to fill the device with strips of that size (a function of n and the effort alone).  A strip is written
                            as one byte-aligned DEFLATE block per 32 KiB; inside it the 32 KiB window slides across
                            those blocks (src/decompress.cpp:178 only requires distance <= bytes written), so
                            larger strips compress better; 32768 makes every DEFLATE block independent */
  uint32_t effort;       /* enum sfh_effort.  SFH_EFFORT_DEFAULT searches the even positions (an odd one takes over its
                            successor's match when its own byte fits in front of it) with both history levels of a hash
                            bucket plus the step-local candidate; SFH_EFFORT_FAST only the newer level (about 2 % more
                            output); SFH_EFFORT_FASTEST drops the step-local candidate as well (about 4 % more than the
                            default on text, more on very repetitive data); SFH_EFFORT_THOROUGH searches every
                            position, in insertion steps of 512 (about 1.3 % less output than the default on text, 2.5 %
                            on mixed data, for a quarter more time); SFH_EFFORT_MAX adds a second hash table keyed by seven
                            bytes to that (two tables of 4096 buckets instead of one of 8192: four far candidates per
                            position; 2.7 % less output than thorough on text, for a third more time);
                            SFH_EFFORT_BEST / _ULTRA / _EXTREME replace the step tables by exact HASH CHAINS, zlib's own
                            structure (every position inserted and searched, the 8 / 16 / 32 most recent positions with
                            its hash tried, nearest first): what closes the gap to zlib -6 on real data, where recency
                            counts for more than on the synthetic text, at a quarter to a tenth of the default's speed;
                            EXTREME is zlib -6's own ratio on the text workload.
                            SFH_EFFORT_RECENT / SFH_EFFORT_RECENT_ALL keep the step tables' search pattern (every other
                            position / every position, three candidates each) but fill the buckets in POSITION ORDER:
                            a bucket holds the latest position with the hash and the one before the latest inserting
                            step, and a position's third candidate is its exact predecessor -- the nearest earlier
                            position with its hash, inside the step or before it.  RECENT_ALL is thorough's pattern (on
                            real bytes max's ratio or better -- machine code +3 points -- for a tenth less time): the
                            effort for real source text and machine code.  RECENT (the default's pattern) is DEPRECATED:
                            measured, it is thorough's ratio at thorough's speed on every workload (round 5), i.e. no
                            point of its own on the speed / ratio curve; it stays accepted and bit-exact, new callers use
                            THOROUGH or RECENT_ALL.  Both rest on the LDS executing the lanes of one returning atomic in
                            ascending order (sfh_lds_order_check) */
  uint32_t chain_depth;  /* 0: what the effort implies.  With a chain effort (SFH_EFFORT_BEST / _ULTRA / _EXTREME) any depth
                            1..255 -- candidates per position, most recent first (the specification's chain_depth): 4 is
                            SFH_EFFORT_MAX's ratio on text and the chains' on real data at 80 K MiB/s.  Must be 0 with the
                            table efforts (this was the `reserved` word: a caller that zeroes it gets what it got) */
} sfh_options;

enum sfh_effort { SFH_EFFORT_DEFAULT = 0, SFH_EFFORT_FAST = 1, SFH_EFFORT_FASTEST = 2, SFH_EFFORT_THOROUGH = 3, SFH_EFFORT_MAX = 4,
                  SFH_EFFORT_BEST = 5, SFH_EFFORT_ULTRA = 6, SFH_EFFORT_EXTREME = 7, SFH_EFFORT_RECENT = 8, SFH_EFFORT_RECENT_ALL = 9 };
/* (SFH_EFFORT_RECENT is deprecated: see the `effort` field above) */

#define SFH_DEFAULT_BLOCK_BYTES 262144u
/* block_bytes = 0 on inputs large enough to fill the device four times over with strips of that size (2048 / 1024 of them):
 * 512 KiB, 1 MiB with SFH_EFFORT_BEST and above */
#define SFH_LARGE_BLOCK_BYTES 524288u
#define SFH_CHAIN_BLOCK_BYTES 1048576u

/* fills *o with defaults: AUTO, final_stream=1, lazy=3, block_bytes=0, effort=SFH_EFFORT_DEFAULT */
void sfh_default_options(sfh_options* o);

int sfh_device_count(void);

/* what hipDeviceProp_t reports for `device` (bench.py prints the HBM peak these imply) */
typedef struct sfh_device_props {
  char name[64];
  char arch[32];             /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
  uint32_t compute_units;
  uint32_t lds_bytes_per_cu; /* maxSharedMemoryPerMultiProcessor */
  uint32_t l2_bytes;
  uint32_t memory_clock_khz;
  uint32_t memory_bus_bits;
  uint32_t clock_khz;        /* clockRate: the shader clock bench.py turns kernel times into cycles with */
  uint64_t total_memory;
} sfh_device_props;
int sfh_get_device_props(int device, sfh_device_props* out);
/* Environment read by sfh_create (diagnostics and tests; none changes a stream): SFH_BATCH_CHUNKS=<n> (32 KiB chunks per batch of
 * the compressor and the decoder, default 32768 = 1 GiB), SFH_INFLATE_SERIAL=1, SFH_K1_STAMPS=1, SFH_FORCE_ORDER_FAIL=1 (below). */
int sfh_create(sfh_ctx** out, int device);
/* The chain efforts (SFH_EFFORT_BEST / _ULTRA / _EXTREME) and SFH_EFFORT_RECENT insert 64 positions into their hash buckets
 * with ONE returning LDS atomic and rely on the LDS executing that wave-instruction's lanes in ascending order where they
 * meet at one address (op 0: ds_wrxchg_rtn_b32, op 1: ds_mskor_rtn_b32) -- measured behaviour of gfx950, not an ISA
 * promise.  This runs the check the library itself runs ONCE PER CONTEXT, inside sfh_create (two launches of well under a
 * millisecond on the context's own stream and one synchronisation there; the verdict is cached, so no compress call -- the
 * asynchronous ones included -- ever blocks or launches anything for it):
 * `blocks` (1..4096) workgroups x `iters` (1..128) insertion steps x five collision densities (the kernel counts in 32 bits:
 * larger arguments are SFH_E_INVALID_ARG) in the match kernel's own access pattern
 * (partial exec masks, sixteen back-to-back instructions by one wave on shared buckets, the other waves reading the
 * table meanwhile), every position compared with the sequential model.  *mismatches == 0: the order holds.  A compress
 * call with one of those efforts on a context whose check failed returns SFH_E_UNSUPPORTED and changes nothing
 * (sfh_last_error says why); every other effort is unaffected.  SFH_FORCE_ORDER_FAIL=1 in the environment at
 * sfh_create makes the library's own check report failure (tests of that branch). */
int sfh_lds_order_check(sfh_ctx* ctx, uint32_t op, uint32_t blocks, uint32_t iters, uint64_t* mismatches, uint64_t* checked);
void sfh_destroy(sfh_ctx* ctx);
const char* sfh_last_error(const sfh_ctx* ctx);

/* worst-case output bytes for n input bytes (any strategy, any container); block_bytes as in sfh_options
 * (SURVEY.md 8(b) signature).  The bound is per 32 KiB DEFLATE block and a strip is a whole number of those, so every
 * valid block_bytes gives the same figure; a block_bytes the compress calls reject (not a multiple of 32768, or above
 * 16 MiB) returns 0. */
size_t sfh_compress_bound(size_t n, uint32_t block_bytes);

/* ---- Seekable gzip: the dictzip random-access table (SFH_DICTZIP) ----
 *   1F 8B 08 04  00 00 00 00  00 FF        the gzip header SFH_GZIP writes, FLG = FEXTRA
 *   XLEN (u16) = 10 + 2 * nseg | 'R' 'A' | LEN (u16) = 6 + 2 * nseg | VER (u16) = 1 | CHLEN (u16) = 32768 | CHCNT (u16) = nseg
 *   nseg x u16: compressed bytes of segment i (= index[i + 1] - index[i]; the last one reaches to the trailer and holds BFINAL)
 *   the raw DEFLATE body, CRC-32, ISIZE: byte for byte what SFH_GZIP writes at block_bytes = 32768 with the same options
 * (all little-endian; nseg = max(1, ceil(n / 32768))).  Every gzip reader inflates the file, dictzip readers seek in it, and
 * sfh_dz_read_index* turns the table back into the segment index of sfh_decompress_ranges*.  XLEN is 16 bits wide, so nseg <=
 * SFH_DZ_MAX_CHUNKS and n <= SFH_DZ_MAX_CHUNKS * 32768 = 1,073,545,216 bytes: the format's limit.  After such a compress call
 * the index, the sub-index and sfh_last_block_bytes() (32768) are as after any other; index[0] is this header's end.
 *
 * sfh_dz_header_bytes: 22 + 2 * nseg for n input bytes, 0 above the limit.
 * sfh_compress_bound_container: the capacity a compress call with `container` needs: for SFH_DICTZIP sfh_compress_bound(n, 32768)
 * + sfh_dz_header_bytes(n) - 10 (the bound counts the gzip header), and 0 for a block_bytes the call would refuse (anything but 0
 * and 32768) or an n above the limit; for the other containers sfh_compress_bound(n, block_bytes); 0 for an unknown container. */
#define SFH_DZ_MAX_CHUNKS 32762u
size_t sfh_dz_header_bytes(size_t n);
size_t sfh_compress_bound_container(size_t n, uint32_t block_bytes, uint32_t container);

/* Host buffers, synchronous.  *out_n = stream bytes.  Inside the call the input goes up, through the kernels and the
 * stream comes down in 64 MiB batches on three streams, so with pinned buffers the call takes about as long as the
 * larger of its two copies (pageable buffers make the copies themselves synchronous). */
int sfh_compress(sfh_ctx* ctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n,
                 const sfh_options* opt);

/* One process, several GPUs: `src` is cut into nctx contiguous shards on 32 KiB boundaries,
 * shard i is compressed by ctxs[i] (normally one ctx per device; the contexts must be distinct) from its own host
 * thread, every shard but the last as a non-final byte-aligned stream, and the streams are concatenated in `dst`
 * -- one valid stream, bit-identical to what a single sfh_compress call writes.  cap >= sfh_compress_bound(n).
 * opt->final_stream applies to the last shard; a container wraps the whole (shard checksums are computed on their
 * devices and combined).  The block index of the whole stream is not assembled (use the per-ctx ones). */
int sfh_compress_multi(sfh_ctx* const* ctxs, int nctx, const void* src, size_t n, void* dst, size_t cap,
                       size_t* out_n, const sfh_options* opt);

/* One process PER GPU (north_star: "RCCL over xGMI only to concatenate the independently-encoded
 * block streams"): every rank compresses its own shard -- whole strips, final_stream = 0 on every rank but the last -- and
 * the byte-aligned streams are put back to back on rank `root`.  No data-path collective: shard legality is
 * /root/reference/src/decompress.cpp:178 (a match only has to stay inside the bytes already written) and :410-415
 * (blocks until BFINAL).
 *
 * sfh_gather_offsets: the host arithmetic.  offsets[r] = first byte of rank r's stream in the concatenation that starts
 * at `base`, offsets[nranks] = its end; SFH_E_DST_TOO_SMALL when that exceeds cap, SFH_E_INVALID_ARG on overflow.
 *
 * sfh_gather_streams: called by EVERY rank of `nccl_comm` (an ncclComm_t of RCCL, passed as a plain pointer; RCCL is bound
 * with dlopen at the first call, so the library itself does not link it).  d_stream / d_size: this rank's stream and its
 * byte count ON THE DEVICE, as sfh_compress_device_async leaves them.  One ncclAllGather of the u64 sizes, one read-back of
 * them (h_sizes[nranks], every rank: the transfers need host counts), then ONE grouped round of ncclSend / ncclRecv --
 * each peer's bytes travel once, point to point over their own xGMI link, straight to d_out + offsets[peer] on the
 * root; the root's own stream is a device copy (none when it already lies at its place).  Everything is enqueued on
 * `stream`, which is synchronised once, for the sizes; the call returns with the transfers in flight.  *out_end (every
 * rank) = end of the concatenation.  d_out is only read on the root; `base` and `cap` (the root's: bytes already in d_out,
 * its capacity) are passed alike by every rank, so that all ranks refuse together -- before anything is posted -- when the
 * streams do not fit.  The exchange carries, beside the size, every rank's base and cap and the root's d_stream / d_out
 * addresses (five u64 per rank): ranks that DISAGREE on base or cap, and a root whose d_stream overlaps the gathered range
 * of d_out without lying exactly at its own place there (a peer's bytes would land on it, or it would be copied onto
 * itself), are SFH_E_INVALID_ARG on EVERY rank alike, still before anything is posted.
 * Contract for what the library cannot see: a failure that strikes ONE rank after the exchange -- the read-back or the
 * stream synchronisation failing, ncclSend / ncclRecv returning an error -- returns on that rank only; its peers are then
 * inside a grouped transfer that cannot complete.  The communicator is broken at that point (as after any failed RCCL
 * call): abort it (ncclCommAbort) on all ranks and build a new one. */
int sfh_gather_offsets(const uint64_t* sizes, int nranks, uint64_t base, uint64_t cap, uint64_t* offsets);
/* ranks of the communicator and this process's rank in it (ncclCommCount / ncclCommUserRank through the same binding) */
int sfh_comm_ranks(void* nccl_comm, int* nranks, int* rank);
int sfh_gather_streams(sfh_ctx* ctx, void* nccl_comm, int root, const void* d_stream, const uint64_t* d_size, void* d_out,
                       uint64_t base, uint64_t cap, uint64_t* h_sizes, uint64_t* out_end, void* stream);

/* Device buffers (d_src 16-byte aligned), enqueued on `stream` (a hipStream_t,
 * NULL = the ctx's own stream); synchronises the stream and returns the size. */
int sfh_compress_device(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap,
                        size_t* out_n, const sfh_options* opt, void* stream);

/* Same, but only enqueues: no host synchronisation.  The stream size is left in
 * device memory at *d_out_n (uint64_t, device pointer, may not be NULL). */
int sfh_compress_device_async(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap,
                              uint64_t* d_out_n, const sfh_options* opt, void* stream);

/* ---- batched compression: `count` independent items, each its own complete stream, in one call ----
 * Item i's stream (raw, or zlib / gzip with its own header and trailer) is byte-identical to what
 * sfh_compress(ctx, item_i, n_i, ..., opt) writes alone; block_bytes = 0 resolves per item, from n_i (so items below
 * 16 MiB get 32 KiB strips).  The items are cut into launch batches of whole items (at most 32768 chunks, 1 GiB of input;
 * SFH_BATCH_CHUNKS lowers it; a larger item gets launch batches of its own) that run the single call's kernels over
 * descriptor tables, so a call on many small items fills the GPU as one large call does.
 * Everything is checked before anything is enqueued: bad options, a null array or pointer, a device source not 16-byte
 * or a device destination not 4-byte aligned, an item above 2^44 bytes and two overlapping destination ranges
 * [dst_i, dst_i + dst_cap[i]) are SFH_E_INVALID_ARG; dst_cap[i] < sfh_compress_bound(src_n[i], 0) is SFH_E_DST_TOO_SMALL.
 * count == 0 is SFH_OK and does nothing.  After a batch call the context has no block index: sfh_index_entries() is 0,
 * sfh_copy_index / sfh_copy_subindex are SFH_E_INVALID_ARG, sfh_last_block_bytes() is 0; sfh_last_stage_ms works.
 *
 * Device buffers, enqueued on `stream` (NULL: the context's), no host synchronisation.  The host arrays are read before
 * the call returns; item i's stream size lands in d_out_n[i] (device memory, uint64). */
int sfh_compress_batch_device_async(sfh_ctx* ctx, size_t count,
                                    const void* const* d_srcs, const uint64_t* src_n,
                                    void* const* d_dsts, const uint64_t* dst_cap,
                                    uint64_t* d_out_n, const sfh_options* opt, void* stream);
/* Host buffers, synchronous: the items travel through pinned staging, packed (one copy per 64 MiB each way, not one per
 * item); out_n[i] on the host. */
int sfh_compress_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n,
                       void* const* dsts, const uint64_t* dst_cap, uint64_t* out_n, const sfh_options* opt);

/* The index of the last call when it was an sfh_compress_batch* call (SFH_E_INVALID_ARG after any other call, or before any):
 * *items = the call's items, *entries = sum over i of (nseg_i + 1), nseg_i = max(1, ceil(n_i / 32768)).  The sub-index has
 * (entries - items) * SFH_SUBINDEX_WORDS words. */
int sfh_batch_index_size(const sfh_ctx* ctx, size_t* items, size_t* entries);
/* Copies that index, item after item: item i's nseg_i + 1 offsets relative to ITS stream's first byte (header included, trailer
 * excluded: the single call's convention), its nseg_i * SFH_SUBINDEX_WORDS sub-index words, and its resolved block_bytes (one
 * uint32 per item).  Any of the three may be NULL.  dst_on_device: device memory, else host.  Synchronises `stream`. */
int sfh_copy_batch_index(sfh_ctx* ctx, uint64_t* index, uint32_t* subindex, uint32_t* block_bytes, int dst_on_device,
                         void* stream);

/* ---- measurement hooks (bench.py, tests) ---- */

/* ---- block index + GPU decompress ----
 * A stream written by sfh_compress* is a sequence of byte-aligned segments, one DEFLATE block per 32 KiB of input
 * (SFH_SEGMENT_BYTES).  The index is the table of their first bytes plus the end of the last one: nseg + 1
 * uint64 offsets into the stream (wrapper header included, trailer excluded).  Segments group into strips of
 * block_bytes of input (sfh_options.block_bytes, sfh_last_block_bytes): no match reaches before its strip, so
 * strips decode independently; inside a strip the Huffman decoding of all segments still runs at once and only
 * the byte copies go segment by segment.  With the index the reference's decompress()
 * (src/decompress.hpp:63-71) runs on the GPU; without it DEFLATE decoding is serial (README.md:5-6).  Any
 * stream with such an index qualifies, e.g. zlib output flushed with Z_FULL_FLUSH every 32 KiB (block_bytes =
 * 32768: every segment independent). */
#define SFH_SEGMENT_BYTES 32768u

/* strip size (sfh_options.block_bytes after defaulting) of the last sfh_compress* call on this ctx; 0 before any */
uint32_t sfh_last_block_bytes(const sfh_ctx* ctx);

/* entries of the index of the last sfh_compress* call on this ctx (segments + 1); 0 before any call */
size_t sfh_index_entries(const sfh_ctx* ctx);
/* copies that index to `dst` (host memory, or device memory if dst_on_device); synchronises `stream` */
int sfh_copy_index(sfh_ctx* ctx, uint64_t* dst, size_t entries, int dst_on_device, void* stream);

/* Sub-index of the last sfh_compress* call: per segment, for each of its 32 regions of 1024 bytes of output
 * (no match of this library's streams crosses them) {bit offset of the region's first token code counted from
 * the segment's first byte, tokens before the region}: SFH_SUBINDEX_WORDS uint32 per segment, all zero for a
 * stored segment.  Optional side information: with it the 32 lanes that decode one segment's Huffman codes side
 * by side are TOLD where their regions start (the decoder checks it against the stream: a wrong sub-index is an
 * error, never wrong output).  Streams from elsewhere have none: their segments are decoded by 32 lanes as well,
 * which find their token boundaries speculatively, block after block (up to four blocks with output per segment
 * plus the empty stored blocks a flush leaves; about 1.5 x the sub-indexed time), and by one lane per segment where
 * a segment is cut into more blocks or is damaged -- the serial decoder itself, statuses included
 * (SFH_INFLATE_SERIAL=1 in the environment of sfh_create: that kernel for every segment). */
#define SFH_SUBINDEX_WORDS 64u
int sfh_copy_subindex(sfh_ctx* ctx, uint32_t* dst, size_t words, int dst_on_device, void* stream);

/* Device buffers (d_src 4-byte, d_index 8-byte, d_dst 16-byte aligned; d_subindex 4-byte aligned or NULL;
 * d_src readable up to the next multiple of 4 bytes, as any device allocation is).
 * nseg must be ceil(dst_n / 32768)
 * (1 for dst_n = 0); segment i decodes stream bytes [index[i], index[i+1]) into dst[i*32768 ...) and must
 * produce exactly that many bytes.  block_bytes: the strip size the stream was written with (a multiple of 32768;
 * 0 = 32768, every segment independent): a match of segment i may reach back to the first byte of its strip,
 * a farther one is InvalidDistance.  Returns SFH_OK when the kernels ran; *status is then the reference's
 * DecompressStatus (0 = Success) of the first failing segment in stream order; dst is complete only on 0.
 * Which status a damaged segment gets: the serial decoder's (starflate::decompress, container.hpp) on the segment's own
 * bytes with a capacity of the segment's output size -- its checks in its order, so a bit field cut short is Error, a code
 * that needs bits behind the segment's end is InvalidLitOrLen / InvalidDistance, distance symbols 30 and 31 are
 * InvalidLitOrLen -- on every path (sub-indexed, index only, batch, range, dictzip, BGZF, recovered index).  With the index
 * alone no byte behind the segment changes the answer.  With a sub-index the region lanes are not held to the segment's last
 * bit: a segment that an index entry cuts short is still decoded from the bytes behind it, and the failure is then the next
 * segment's.  A match may reach the earlier segments of its strip as it may reach earlier output in a stream.
 * Where a segment is not a stream: a final block that ends short of the segment's size is SrcTooSmall (the index promised
 * more); well-formed non-final blocks that end on the segment's last bits are Success when they made its size, else
 * SrcTooSmall (alone they would be InvalidBlockHeader: no header follows); a segment of no bytes is InvalidBlockHeader.
 * Synchronises `stream` (NULL = the ctx's own).
 * Scratch: the decoder keeps 4 bytes of tokens per output byte -- of ONE batch of whole strips, at most 1 GiB of output (round
 * 6; before: of the whole call): 4 GiB at most whatever dst_n is (sfh_last_decode_scratch_bytes), the two kernels alternating
 * batch after batch on the stream; bytes and status are those of one pass over everything
 * (/root/reference/src/decompress.cpp:197-242 semantics: the first failing block in stream order).
 * The call is an sfh_decompress_batch_device_async call of one raw item followed by one synchronisation: one set of kernels
 * and one geometry serve both.  What that means for a single stream, against the implicit-geometry kernels it ran before:
 *   - the call builds and uploads a descriptor table, 48 bytes per segment plus 8 per strip (about 0.15 % of the output), in
 *     pinned host memory and on the device -- so it can fail with SFH_E_NOMEM for that table;
 *   - before it fills the pinned table it waits, on the host, for the previous call's table copy to have read it;
 *   - it launches k_inflate_head (for a raw item: nothing but a cleared wrapper status) in front of the token kernels and
 *     k_inflate_fold behind the byte kernels, where it launched k_inflate_status.
 * Bytes, statuses, the first failing segment sfh_last_error names and the scratch are unchanged. */
int sfh_decompress_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                          const uint32_t* d_subindex, size_t nseg, void* d_dst, size_t dst_n, uint32_t block_bytes,
                          uint32_t* status, void* stream);
/* Host buffers: H2D (stream + index [+ sub-index, may be NULL]), decode, D2H. */
int sfh_decompress(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* index, const uint32_t* subindex,
                   size_t nseg, void* dst, size_t dst_n, uint32_t block_bytes, uint32_t* status);

/* ---- batched decompression: `count` independent streams, each decoded into its own buffer, in one call ----
 * Item i: stream srcs[i] of src_n[i] bytes (raw, or zlib / gzip: `container`, the same for every item), decoded into exactly
 * dst_n[i] bytes at dsts[i]; its DecompressStatus into status[i].
 * index: every item's segment index, item after item in sfh_copy_batch_index's layout (nseg_i + 1 offsets into ITS stream,
 *   nseg_i = max(1, ceil(dst_n[i] / 32768))), or NULL when every dst_n[i] <= 32768: each item is then one segment, from the
 *   end of its wrapper header to src_n[i] minus its trailer (pages that other tools wrote).
 * subindex: flattened the same way (SFH_SUBINDEX_WORDS per segment), or NULL.  block_bytes: per item (0 = 32768), or NULL =
 *   32768 for all.
 * A raw item's bytes and status are those of sfh_decompress_device on it alone with the same index, sub-index and block_bytes;
 * a wrapped one's status is include/starflate/container.hpp's decompress(src_i, dst_i, container): the wrapper (SrcTooSmall
 * for a stream too short for it; gzip's FEXTRA / FNAME / FCOMMENT / FHCRC are read), ISIZE against dst_n[i], the body, then
 * the Adler-32 / CRC-32 (a mismatch is Error); with an index, a wrapped item's entry 0 must be the header's end (else Error;
 * a raw item's entry 0 is not checked, as in sfh_decompress_device).  A gzip item with ISIZE below dst_n[i] is decoded into
 * its first ISIZE bytes, as container.hpp does; a wrapped body that ends short of its output is Error.  One
 * item's failure changes no other item's bytes or status, and nothing is written outside [dsts[i], dsts[i] + dst_n[i]).
 * Refused before anything is enqueued (SFH_E_INVALID_ARG): a null context or an unknown container (also with count == 0), a
 * null array (count > 0), a device pointer out of the single decoder's alignment (src 4, dst 16, index 8, sub-index 4,
 * status 4), dst_n above 2^44, a bad block_bytes (not a multiple of 32768, or above 16 MiB), overlapping destination ranges
 * (a destination of no bytes overlaps nothing),
 * no index while some dst_n[i] > 32768, a sub-index without an index, more than 2^31 - 1 segments.  count == 0: SFH_OK.
 * The items run in launch batches of whole items (at most SFH_BATCH_CHUNKS segments; a larger item in batches of its own, cut
 * at its strips: max(sps, SFH_BATCH_CHUNKS / sps * sps) segments each, sps = block_bytes / 32768), so the token scratch is
 * that of one batch
 * (sfh_last_decode_scratch_bytes, at most 4 GiB).  Afterwards the context has no index, as after sfh_decompress*;
 * sfh_last_inflate_ms sums both stages over the launch batches.
 *
 * Device buffers, enqueued on `stream` (NULL: the context's), no host synchronisation; the host arrays (src_n, dst_n,
 * block_bytes) are read before the call returns; status: device uint32[count]. */
int sfh_decompress_batch_device_async(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                      const uint64_t* d_index, const uint32_t* d_subindex, void* const* d_dsts,
                                      const uint64_t* dst_n, const uint32_t* block_bytes, uint32_t container,
                                      uint32_t* d_status, void* stream);
/* Host buffers, synchronous (through pinned staging, as sfh_compress_batch): status[i] on the host; dsts[i] is written only
 * when status[i] == 0. */
int sfh_decompress_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n,
                         const uint64_t* index, const uint32_t* subindex, void* const* dsts, const uint64_t* dst_n,
                         const uint32_t* block_bytes, uint32_t container, uint32_t* status);

/* ---- random access: byte ranges of one indexed stream's output, decoded for roughly what they hold ----
 * The stream, its index, sub-index (or NULL) and block_bytes are sfh_decompress_device's; total_n is the stream's whole
 * output size and nseg == max(1, ceil(total_n / 32768)).  Range r is output bytes [offsets[r], offsets[r] + lengths[r]); with
 * status[r] == 0, dsts[r][0, lengths[r]) holds exactly those bytes of what sfh_decompress_device writes for the whole
 * stream.  Offsets, lengths and destination addresses need no alignment (ranges can be gathered into a packed buffer); source
 * ranges may overlap each other, destination ranges [dsts[r], dsts[r] + lengths[r]) may not.  A range of no bytes is status 0
 * and writes nothing.
 * Work: the DECODE SPAN of a range is the segments from the first one of the strip (block_bytes of output) that holds its
 * first byte to the one that holds its last byte.  Only the spans' segments get tokens and are walked by the byte stage; those
 * in front of the range's first byte are resolved in LDS only (a match may reach back to the strip's start), and nothing of
 * them reaches global memory but their tokens.  With block_bytes = 32768 a range inside one segment costs that segment.  Every
 * range is decoded by itself: ranges that share a strip each pay for their span.  The spans run in launch batches of whole
 * strips, at most SFH_BATCH_CHUNKS segments each (a larger strip is a batch of its own): the token scratch is one batch's
 * (sfh_last_decode_scratch_bytes); sfh_last_inflate_ms sums both stages over the batches.
 * status[r]: the DecompressStatus of the first failing segment of r's decode span in stream order, 0 when none fails; a
 * segment must produce exactly its 32768 bytes (the stream's last one its remainder), and a wrong sub-index is an error, never
 * wrong bytes.  Damage outside a range's decode span changes neither its bytes nor its status; one range's failure changes no
 * other range.  No checksum is verified (a range cannot verify one).  The stream may be wrapped: the index's offsets include
 * the header, and the trailer is never read.  Nothing is written outside [dsts[r], dsts[r] + lengths[r]).
 * Refused before anything is enqueued (SFH_E_INVALID_ARG): a null context; with count > 0 a null stream, index or array, or a
 * null destination with a non-zero length; offsets[r] + lengths[r] above total_n (or overflowing); total_n above 2^44; nseg
 * not matching total_n; a bad block_bytes; a device pointer out of alignment (d_src 4, d_index 8, d_subindex 4, d_status 4);
 * overlapping destinations; decode spans of more than 2^31 - 1 segments altogether.  count == 0: SFH_OK.  Afterwards the
 * context has no index, as after sfh_decompress*.
 *
 * Device buffers, enqueued on `stream` (NULL: the context's), no host synchronisation; the host arrays (offsets, lengths,
 * d_dsts) are read before the call returns; d_status: device uint32[count]. */
int sfh_decompress_ranges_device_async(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                                       const uint32_t* d_subindex, size_t nseg, uint64_t total_n, uint32_t block_bytes,
                                       size_t count, const uint64_t* offsets, const uint64_t* lengths, void* const* d_dsts,
                                       uint32_t* d_status, void* stream);
/* One range; synchronises `stream`, *status on the host. */
int sfh_decompress_range_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_index,
                                const uint32_t* d_subindex, size_t nseg, uint64_t total_n, uint32_t block_bytes,
                                uint64_t offset, uint64_t length, void* d_dst, uint32_t* status, void* stream);
/* Host buffers, synchronous: the stream, index, sub-index and destinations on the host, status[count] on the host; dsts[r] is
 * written only when status[r] == 0.  The whole stream is NOT uploaded: for every decode span only its stream bytes go up --
 * from the smallest to the largest of its index entries (in a sound index: [index[first], index[last + 1])), clipped to
 * src_n and rounded out to 16 bytes -- packed, piece after piece, through the pinned staging, with the span's index entries
 * and sub-index words.  The index offsets stay offsets into the stream: every row of a span carries a stream base that
 * points as far in front of the span's piece as the piece's first byte lies in the stream (a per-span InflateSeg.src), and
 * a stream size that ends with the piece, so what the kernels read at base + offset is the uploaded copy. */
int sfh_decompress_ranges(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* index, const uint32_t* subindex,
                          size_t nseg, uint64_t total_n, uint32_t block_bytes, size_t count, const uint64_t* offsets,
                          const uint64_t* lengths, void* const* dsts, uint32_t* status);

/* ---- reading a dictzip table: the index from the file's own header, no side information and no scan ----
 * The gzip header of `src` is parsed (magic, CM; the FEXTRA subfields up to 'RA', others may stand before and behind it; FNAME,
 * FCOMMENT and FHCRC skipped; no read beyond src_n) and the table's sizes are summed into the index: index[0] = the header's
 * end, index[i + 1] = index[i] + size[i], index[nseg] = src_n - 8, the trailer's first byte -- so the last segment takes in
 * what lies between the table's end and the trailer (dictzip(1) leaves its empty final block there).  info->total_n = ISIZE,
 * info->nseg = max(1, CHCNT), info->header_bytes = index[0].
 * SFH_E_NOT_INDEXABLE, nothing written: no FEXTRA, no 'RA' subfield, VER != 1, or CHLEN != 32768 (the indexed decoder's segments
 *   are 32 KiB: files of dictzip's own default chunk length go to sfh_inflate_stream*).
 * SFH_OK with info->status = 5 (SrcTooSmall): a stream too short for its header and trailer (below 18 bytes, or a file name,
 *   comment or header CRC that does not end in front of the trailer).
 * SFH_OK with info->status = 1 (Error): bad magic or CM, XLEN or a subfield overrunning, LEN != 6 + 2 * CHCNT, CHCNT != max(1,
 *   ceil(ISIZE / 32768)) (CHCNT == 0 with ISIZE == 0 reads as one empty segment), the sizes' sum reaching past src_n - 8.
 *   With a non-zero status the other fields are 0 and the index is not written.
 * SFH_E_DST_TOO_SMALL: index_cap < nseg + 1 (SFH_DZ_MAX_CHUNKS + 1 entries always suffice); SFH_E_INVALID_ARG: a null pointer.
 * sfh_dz_read_index: host bytes, no context, no device: arithmetic on the header.
 * sfh_dz_read_index_device: device bytes (d_src 4-byte, d_index 8-byte aligned), one workgroup (k_dz_index), then one read-back
 *   of the info: one synchronisation of `stream` (NULL = the ctx's own). */
typedef struct sfh_dz_info {
  uint64_t total_n;
  uint32_t nseg, header_bytes, status, reserved;
} sfh_dz_info;
int sfh_dz_read_index(const void* src, size_t src_n, sfh_dz_info* info, uint64_t* index, size_t index_cap);
int sfh_dz_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_dz_info* info, uint64_t* d_index,
                             size_t index_cap, void* stream);
/* A dictzip file decoded with its own table: the index is read (as above), then the file runs as one SFH_GZIP item of
 * sfh_decompress_batch* with that index and block_bytes = 32768 -- the wrapper, ISIZE and the CRC-32 are verified exactly as
 * there.  *dst_n_out = ISIZE; ISIZE > dst_cap is SFH_E_DST_TOO_SMALL; a table that does not parse gives its status (1 or 5) in
 * *status with nothing decoded; SFH_E_NOT_INDEXABLE as above, nothing decoded.  d_src 4-byte, d_dst 16-byte aligned;
 * synchronises `stream`.  sfh_decompress_dz: host buffers (H2D, the same, D2H of dst when *status is 0).
 * sfh_decompress_dz_ranges: host buffers; the header is read on the host, then sfh_decompress_ranges runs with that index: only
 * the decode spans' bytes are uploaded.  A table that does not parse gives every range its status.  For a file on the device:
 * sfh_dz_read_index_device, then sfh_decompress_ranges_device_async. */
int sfh_decompress_dz_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                             uint32_t* status, void* stream);
int sfh_decompress_dz(sfh_ctx* ctx, const void* src, size_t src_n, void* dst, uint64_t dst_cap, uint64_t* dst_n_out,
                      uint32_t* status);
int sfh_decompress_dz_ranges(sfh_ctx* ctx, const void* src, size_t src_n, size_t count, const uint64_t* offsets,
                             const uint64_t* lengths, void* const* dsts, uint32_t* status);

/* ---- BGZF: the blocked gzip of bgzip / htslib (BAM, BCF, tabix), written and read ----
 * A series of complete gzip members, each stating its own size, closed by a fixed empty member (all little-endian):
 *   member: 1F 8B 08 04 | MTIME 0 | XFL 0 | OS FF | XLEN 06 00 | 'B' 'C' 02 00 | BSIZE (u16) = the member's bytes - 1
 *           raw DEFLATE body, last block BFINAL | CRC-32 of the member's input | ISIZE (u32)
 *   EOF:    1F 8B 08 04 00 00 00 00 00 FF 06 00 42 43 02 00 1B 00 03 00 00 00 00 00 00 00 00 00  (28 bytes)
 * THE WRITER puts 32768 input bytes into every member (the last one holds the remainder), one member per chunk of the
 * compressor -- a stored chunk, 37504 + 26 bytes, still fits BSIZE; two chunks would not -- then the EOF member; an input of 0
 * bytes gives the EOF member alone, as bgzip writes it.  Defining property: with the input cut into slices of 32768 bytes the
 * file is, for every slice, the 18-byte header above, bytes [10:] of what sfh_compress(slice, container = SFH_GZIP, the same
 * options) writes alone (body, CRC-32, ISIZE) with BSIZE to match, and the EOF member behind the last.
 * Options: container must be SFH_RAW (the call is the wrapper), final_stream 1, block_bytes 0 or 32768 (0 means 32768); every
 * strategy, effort, lazy and chain_depth of sfh_compress.  Anything else is SFH_E_INVALID_ARG before anything is enqueued;
 * cap < sfh_bgzf_bound(n) is SFH_E_DST_TOO_SMALL.  sfh_bgzf_bound(n) = max(1, ceil(n / 32768)) * (sfh_compress_bound(32768, 0)
 * + 26) + 28.  Alignment as sfh_compress_device (d_src 16, d_dst 4).  The file's size is not limited: launch batches carry on
 * as in the single-stream call.  sfh_compress_bgzf_device_async makes no host synchronisation (*d_out_n: the file's bytes).
 * After the call the context holds no block index (sfh_index_entries() is 0), as after a batched call.
 * sfh_compress_bgzf: host buffers, staged and pipelined like sfh_compress. */
size_t sfh_bgzf_bound(size_t n);
int sfh_compress_bgzf_device_async(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap, uint64_t* d_out_n,
                                   const sfh_options* opt, void* stream);
int sfh_compress_bgzf_device(sfh_ctx* ctx, const void* d_src, size_t n, void* d_dst, size_t cap, size_t* out_n,
                             const sfh_options* opt, void* stream);
int sfh_compress_bgzf(sfh_ctx* ctx, const void* src, size_t n, void* dst, size_t cap, size_t* out_n, const sfh_options* opt);
/* THE READER finds the members from the file alone.  A member starts where bytes 0..2 are 1F 8B 08 and FLG has FEXTRA; its
 * extra field is walked subfield by subfield for 'B' 'C' with SLEN 2 (others may stand before and behind it); it is BSIZE + 1
 * bytes long and its ISIZE is its last four bytes.  FNAME, FCOMMENT and FHCRC are the gzip decoder's.
 * member_off[0 .. members] = the first byte of every member (the EOF member and any other empty member count) and src_n;
 * out_off[0 .. members] = the prefix sums of ISIZE, so out_off[members] = info->total_n.  info->has_eof: the last member is byte
 * for byte the EOF member (its absence is no error; htslib only warns).  src_n == 0: no members, status 0.
 * info->status = 5 (SrcTooSmall): a member's header (12 bytes and its extra field) or its BSIZE + 1 bytes reach past src_n;
 * 1 (Error): bad magic or CM at a member's start, FEXTRA clear, no 'BC' subfield, a subfield overrunning XLEN, BSIZE + 1 below
 * the member's header plus 8.  With a non-zero status the counts are 0 and the arrays are not written.
 * SFH_E_DST_TOO_SMALL: cap < members + 1 (the arrays hold cap entries each; info then carries the counts, nothing else is
 * written); SFH_E_INVALID_ARG: a null pointer.
 * sfh_bgzf_read_index: host bytes, no context, no device: member after member.
 * sfh_bgzf_read_index_device: device bytes (d_src 4-byte, the arrays 8-byte aligned).  No lane chases BSIZE from member to
 *   member: every byte position that parses as a member's head is a node, pointer jumping from position 0 ranks the nodes the
 *   chain reaches ("BGZF"), and a head-shaped pattern inside compressed data is a node nobody reaches.  Two
 *   synchronisations of `stream` (NULL = the ctx's own) whatever the file holds: the node count, then the info. */
typedef struct sfh_bgzf_info {
  uint64_t total_n;
  uint32_t members, max_isize, has_eof, status;
} sfh_bgzf_info;
int sfh_bgzf_read_index(const void* src, size_t src_n, sfh_bgzf_info* info, uint64_t* member_off, uint64_t* out_off, size_t cap);
int sfh_bgzf_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_bgzf_info* info, uint64_t* d_member_off,
                               uint64_t* d_out_off, size_t cap, void* stream);
/* A BGZF file decoded.  The index is read (as above); with info.max_isize <= 32768 every member is one segment of the indexed
 * decoder and one index-free SFH_GZIP item of sfh_decompress_batch*: its wrapper, ISIZE, body and CRC-32 count exactly as
 * there for that member alone, in launch batches of at most SFH_BATCH_CHUNKS members.  *status = the DecompressStatus of the
 * first failing member in file order, or 0; a file whose index fails gives that status and nothing is decoded.  *dst_n_out =
 * total_n; total_n > dst_cap is SFH_E_DST_TOO_SMALL.  d_src 4-byte, d_dst 16-byte aligned; three synchronisations of `stream`.
 * A member above 32768 bytes (bgzip and htslib write 65280, the format allows 65536): sfh_decompress_bgzf_device returns
 * SFH_E_NOT_INDEXABLE and decodes nothing.
 * sfh_decompress_bgzf_wide_device reads EVERY conforming BGZF file, ISIZE <= 65536 per member: same arguments, alignment,
 * synchronisations, *status and messages.  A file without a member above 32768 bytes takes the path above, launch for launch.
 * A file with one is decoded as a whole on the decoder's WIDE ROWS: a member is still one segment of the same kernels, built a
 * second time for rows of 65536 output bytes and 65536 tokens (the speculative wave follows 8 blocks with output per member
 * instead of 4; the lane-serial kernel stands behind it as ever), with two checksum partials per member.  A wide member's
 * tokens take 256 KiB, so a launch batch holds SFH_BATCH_CHUNKS / 2 members and sfh_last_decode_scratch_bytes keeps its bound.
 * A member claiming more than 65536 bytes is not BGZF: SFH_E_NOT_INDEXABLE, nothing decoded.
 * sfh_decompress_bgzf (host buffers) walks on the host and sends the file up and through the device call that fits its widest
 * member -- at most 32768 bytes: sfh_decompress_bgzf_device; up to 65536: sfh_decompress_bgzf_wide_device -- and dst is
 * written only when *status is 0.  Only gzip members with a 'BC' field that claim more than 65536 bytes (not BGZF) still run as
 * the items of sfh_inflate_stream_batch (SFH_GZIP, dsts[i] = dst + out_off[i], dst_cap[i] = ISIZE_i), the first non-zero item
 * status in order being *status (INTEGRATION.md 1.4 has the rates). */
int sfh_decompress_bgzf_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                               uint32_t* status, void* stream);
int sfh_decompress_bgzf_wide_device(sfh_ctx* ctx, const void* d_src, size_t src_n, void* d_dst, uint64_t dst_cap, uint64_t* dst_n_out,
                                    uint32_t* status, void* stream);
int sfh_decompress_bgzf(sfh_ctx* ctx, const void* src, size_t src_n, void* dst, uint64_t dst_cap, uint64_t* dst_n_out,
                        uint32_t* status);
/* ---- BGZF random access: byte ranges of a BGZF file's output, decoded for the members that hold them ----
 * The file and its index (member_off, out_off, info: sfh_bgzf_read_index*, reusable across calls).  Range r is output bytes
 * [offsets[r], offsets[r] + lengths[r]); with status[r] == 0, dsts[r][0, lengths[r]) holds exactly those bytes of what
 * sfh_decompress_bgzf_wide_device writes for the whole file.  Offsets, lengths and destination addresses need no alignment
 * (ranges can be gathered into a packed buffer); source ranges may overlap each other, destination ranges [dsts[r], dsts[r] +
 * lengths[r]) may not.  A range of no bytes is status 0 and writes nothing.
 * Work: members have no fixed size, so the member of an output byte is a binary search in out_off, run on the device.  The
 * DECODE SPAN of a range is exactly the members it touches -- first = the smallest i with out_off[i + 1] > offset, last = the
 * smallest j with out_off[j + 1] >= offset + length, empty members between them included -- because no match reaches before
 * its member: a 4 KiB record costs one or two members.  Every member of a span is one row of the indexed decoder, narrow
 * (32768) with info->max_isize <= 32768, else wide (65536), for the file as a whole; the rows get tokens and the byte stage
 * writes of each only its window.  Every range is decoded by itself: ranges that share a member each pay for it.  The rows
 * run in launch batches of SFH_BATCH_CHUNKS (wide: SFH_BATCH_CHUNKS / 2) rows, a span may cross a batch boundary, and the token
 * scratch is one batch's (sfh_last_decode_scratch_bytes).
 * Verified per member of a span: its gzip wrapper, that its ISIZE equals its indexed size, and that its body decodes to
 * exactly that many bytes.  NO checksum is verified: a member's decoded bytes never reach global memory as a whole, so a
 * range cannot verify a CRC-32.  status[r]: the DecompressStatus of the first failing member of r's span in file order, a
 * member's wrapper before its body; 0 when none fails.  Damage outside a range's span changes neither its bytes nor its
 * status; one range's failure changes no other range; nothing is written outside [dsts[r], dsts[r] + lengths[r]).  An index or
 * info that disagrees with the file ends in a status (a member that does not lie inside the file, or whose indexed size
 * exceeds the row width, is Error and nothing of it is read; a range that ends behind out_off[members] is Error): never a read
 * beyond src_n or a write outside a destination.  The arrays must hold info->members + 1 entries.
 * Refused (SFH_E_INVALID_ARG) before anything is enqueued: a null context; with count > 0 a null file, index array (device
 * call), info, array or status, or a null destination with a non-zero length; a device pointer out of alignment (d_src 4,
 * d_member_off 8, d_out_off 8, d_status 4); offsets[r] + lengths[r] above info->total_n (or overflowing); overlapping
 * destinations; count above 2^31 - 1.  Spans of more than 2^31 - 1 rows altogether: SFH_E_INVALID_ARG as soon as the planner's
 * row total is known (the device call: behind its first synchronisation, before any decoder kernel is enqueued).
 * info->max_isize > 65536: SFH_E_NOT_INDEXABLE.  info->status != 0: every range gets that status, nothing is decoded.
 * count == 0: SFH_OK.  Afterwards the context has no index, as after sfh_decompress*.
 *
 * sfh_decompress_bgzf_ranges_device: device buffers, on `stream` (NULL: the context's).  TWO host synchronisations: the row
 * total (it sizes the row tables, the segment records and the number of launch batches), then the end of the call.  The
 * statuses stay on the device: d_status, device uint32[count].
 * sfh_decompress_bgzf_ranges: host buffers, synchronous, status[count] on the host; dsts[r] is written only when status[r]
 * == 0.  member_off / out_off / info may all be NULL (all three or none): the members are walked on the host first
 * (sfh_bgzf_read_index), and a file that does not parse gives every range the walk's status.  The whole file is NOT uploaded:
 * for every span only its members' bytes [member_off[first], member_off[last + 1]) go up, clipped to src_n and rounded out
 * to 16 bytes, packed piece after piece through the pinned staging; every row of a span carries a file base that points as far
 * in front of the span's piece as the piece's first byte lies in the file (a per-span InflateSeg.src), so member offsets stay
 * offsets into the file and what the kernels read is the uploaded copy.  The index (16 bytes per member) goes up whole. */
int sfh_decompress_bgzf_ranges_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const uint64_t* d_member_off,
                                      const uint64_t* d_out_off, const sfh_bgzf_info* info, size_t count, const uint64_t* offsets,
                                      const uint64_t* lengths, void* const* d_dsts, uint32_t* d_status, void* stream);
int sfh_decompress_bgzf_ranges(sfh_ctx* ctx, const void* src, size_t src_n, const uint64_t* member_off, const uint64_t* out_off,
                               const sfh_bgzf_info* info, size_t count, const uint64_t* offsets, const uint64_t* lengths,
                               void* const* dsts, uint32_t* status);
/* Virtual offsets, as tabix and BAI indexes state them: v = coffset << 16 | uoffset.  Host arithmetic on a host index
 * (member_off, out_off: members + 1 entries each), no context, no device.
 * sfh_bgzf_voffsets_to_offsets: v -> out_off[i] + uoffset, where member_off[i] == coffset (a binary search) and uoffset <= the
 * member's output bytes; coffset == member_off[members] with uoffset == 0 -> total_n; anything else -> UINT64_MAX in that
 * slot, and the call still returns SFH_OK.
 * sfh_bgzf_offsets_to_voffsets: o -> the member that holds byte o (the span rule's `first`: never an empty member for a byte
 * that exists) and o's place in it; total_n -> member_off[members] << 16; o above total_n -> UINT64_MAX.  So
 * to_offsets(to_voffsets(o)) == o for every o in [0, total_n].
 * SFH_E_INVALID_ARG: a null index array, or with count > 0 a null array. */
int sfh_bgzf_voffsets_to_offsets(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, size_t count,
                                 const uint64_t* voffsets, uint64_t* offsets);
int sfh_bgzf_offsets_to_voffsets(const uint64_t* member_off, const uint64_t* out_off, uint32_t members, size_t count,
                                 const uint64_t* offsets, uint64_t* voffsets);

/* ---- ZIP archives (.zip, .npz, .jar, .whl, .docx, torch.save): stored and deflated entries, written and read ----
 * (APPNOTE 6.3; all little-endian)
 *   local header  50 4B 03 04 | need flags method time date | CRC-32 csize usize | name_len extra_len | name extra | data
 *   directory     50 4B 01 02 | made need flags method time date | CRC-32 csize usize | name_len extra_len comment_len | disk
 *                 attributes | local_off | name extra comment          (one record per entry, after the last entry's data)
 *   end record    50 4B 05 06 | disks | entries | cd_size cd_off | comment; with saturated fields the ZIP64 end record
 *                 (50 4B 06 06) and its locator (50 4B 06 07) stand in front of it
 * THE READER.  The end record is the last position in the file's final 22 + 65535 bytes that holds the signature and whose
 * comment ends the file; the directory is walked record by record from cd_off and must pass exactly `entries` records and end
 * exactly where the (ZIP64) end record starts (archives with prepended data, multi-disk archives and a ZIP64 end record with
 * an extensible data sector are Error).  An entry's sizes, CRC-32, method and flags are the directory's -- saturated sizes and
 * offsets from its 0x0001 extra subfield -- so entries with a data descriptor need nothing special; its local header only
 * places the data: data_off = local_off + 30 + the LOCAL header's name and extra lengths.
 * info->status: 0; 5 (SrcTooSmall): src_n < 22; 1 (Error): every other structural failure.  With a non-zero status the counts
 * are 0 and the table is not written.
 * entry.status: 0; 5: the local header or [data_off, data_off + csize) reaches past cd_off; 1: no local signature, or a
 * stored entry with csize != usize; SFH_ZIP_ENTRY_UNSUPPORTED -- a per-entry code, never a DecompressStatus, the counterpart of
 * SFH_ITEM_NOT_INDEXABLE --: a method other than 0 and 8, or flag bit 0, 5, 6 or 13 (encryption, patch data).
 * name_off: the name's position in the FILE (in the directory record).  out_off[i]: the running sum of (usize + 15) & ~15 --
 * the packed layout in which every entry starts 16-byte aligned; total_out = its end.
 * sfh_zip_read_index: host bytes, no context, no device.  SFH_E_DST_TOO_SMALL with the counts filled when cap < info->entries
 *   (nothing else written); SFH_E_INVALID_ARG: a null pointer.
 * sfh_zip_read_index_device: device bytes (d_src 4-byte aligned), the table on the HOST.  The file's tail (at most 22 + 65535 +
 *   76 bytes), then the directory are copied down and walked there by the same code; the table goes up, k_zip_locals reads every
 *   local header on the device, the table comes back: two synchronisations of `stream` (NULL = the ctx's own) when the directory
 *   lies inside the tail, else three, whatever the archive holds.  The directory is a compact table at a stated place: there is no device walk of it ("ZIP"). */
#define SFH_ZIP_ENTRY_UNSUPPORTED 0xFFFFFFF9u
typedef struct sfh_zip_info {
  uint64_t entries, cd_off, cd_size, total_out;
  uint32_t zip64, status;
} sfh_zip_info;
typedef struct sfh_zip_entry { /* 64 bytes */
  uint64_t local_off, data_off, csize, usize, out_off, name_off;
  uint32_t crc32, status;
  uint16_t method, flags, name_len, pad;
} sfh_zip_entry;
int sfh_zip_read_index(const void* src, size_t src_n, sfh_zip_info* info, sfh_zip_entry* entries, size_t cap);
int sfh_zip_read_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, sfh_zip_info* info, sfh_zip_entry* entries, size_t cap,
                              void* stream);
/* Decodes `count` entries of the file -- any subset of its index, in any order, an entry twice into two destinations if the
 * caller likes -- entry i into d_dsts[i]; status[i] (host) is its DecompressStatus, or the entry's own non-zero index status,
 * which it keeps.  No entry byte is copied or realigned on the way: an item of the decoders is the file with the entry's body
 * range.  Method 0: k_zip_store, a gather copy in 16-byte stores.  Method 8: the index-free decoder of sfh_decompress_any_batch*
 * (raw) -- every archive written here and every entry of at most 32 KiB takes it; an entry it finds not indexable goes through
 * the stream decoder of sfh_inflate_stream_batch* with a capacity of usize, and so does an entry whose segments come up short
 * of what usize promised.  A body that ends in order with fewer than usize bytes is 1 (Error); one that holds more than usize
 * bytes is 4 (DstTooSmall: the serial decoder's status for a destination of usize bytes, and nothing is written behind them);
 * usize above dst_cap[i] is 4 as well, and every entry that decoded has its CRC-32 computed on the device from its
 * output and compared with the directory's: a mismatch is 1.  An empty entry's CRC-32 is 0.  The table is the caller's: an entry
 * whose data range does not lie inside src_n is 5, and nothing of it is read; an entry of 4 GiB or more is
 * SFH_ZIP_ENTRY_UNSUPPORTED here (the checksum fold counts an entry's bytes in 32 bits).
 * One entry's failure changes no other entry's bytes or status; nothing is written outside [d_dsts[i], d_dsts[i] + dst_cap[i]),
 * and for an entry that fails nothing is promised about its own destination.  Refused with SFH_E_INVALID_ARG before anything is
 * enqueued: a null ctx; with count > 0 a null file or array, d_src not 4-byte or a destination not 16-byte aligned, a null
 * destination with dst_cap > 0, overlapping destinations, more than 2^31 - 1 entries.  count == 0: SFH_OK.  Host
 * synchronisations of `stream`: those of the two drivers (sfh_decompress_any_batch_device; sfh_inflate_stream_batch_device
 * only when an entry needs it) and one for the checksums: not more with more entries.  Scratch: the drivers'.  Afterwards the ctx
 * holds no index.  sfh_last_recover_stats / sfh_last_stream_stats describe the deflated entries' decode (zeros where a driver
 * did not run).
 * sfh_decompress_zip: host buffers; entries == NULL: the index is read here (sfh_zip_read_index) and entry i of it goes to
 * dsts[i] (count must then be its entries; a file whose index fails gives every status that failure).  The file goes up whole,
 * the entries are decoded into the packed layout of their rounded sizes and only those with status 0 are copied back. */
int sfh_decompress_zip_device(sfh_ctx* ctx, const void* d_src, size_t src_n, const sfh_zip_entry* entries, size_t count,
                              void* const* d_dsts, const uint64_t* dst_cap, uint32_t* status, void* stream);
int sfh_decompress_zip(sfh_ctx* ctx, const void* src, size_t src_n, const sfh_zip_entry* entries, size_t count, void* const* dsts,
                       const uint64_t* dst_cap, uint32_t* status);
/* THE WRITER: `count` items, each a deflated entry, in one archive that unzip and zipfile open.  Defining property: for every
 * item, in order, the archive holds the local header -- version needed 20, flags 0x0800 (UTF-8 names), method 8, time 0, date
 * 0x0021 (1980-01-01: deterministic, like gzip's MTIME 0), CRC-32, sizes, the name, no extra field -- followed byte for byte by
 * what sfh_compress_batch writes for that item with container = SFH_RAW and the same options; then one directory record per item
 * (version made by 20, no extra, no comment, attributes 0) and the 22-byte end record, with more than 65535 entries the ZIP64
 * end record and locator (version needed 45) in front of it and the classic count saturated.
 * The bodies are compressed one launch batch of whole items at a time (at most SFH_BATCH_CHUNKS chunks; a larger item alone)
 * into context scratch of that batch's bound and packed behind each batch, so the scratch is one batch's.  The bound is per
 * 32 KiB chunk, 37504 bytes, whatever an item holds: an item of one byte takes a slot of that size and two 32 KiB pieces of the
 * pack's launch, so a launch batch of 32768 tiny items (thousands of scalars of an .npz) has 1.2 GB of scratch; SFH_BATCH_CHUNKS
 * lowers it.
 * opt: container must be SFH_RAW and final_stream 1; every strategy, effort, lazy, chain_depth and block_bytes of the batch call.
 * SFH_E_INVALID_ARG before anything is enqueued: an empty name or one above 65535 bytes; an item of 2^32 - 1 bytes or more; local
 * parts whose BOUNDS together reach 2^32 (offsets are not known before an asynchronous call, which cannot fail afterwards;
 * ZIP64 offsets in the writer are out of scope); the batch call's own refusals (d_srcs 16-byte, d_dst 4-byte aligned).
 * cap < sfh_zip_bound(...) is SFH_E_DST_TOO_SMALL.  sfh_zip_bound = the sum over the items of 30 + name_len + sfh_compress_bound(n,
 * 0), plus the sum of 46 + name_len, plus 22 + 76 (0: the sum overflows).  count == 0 writes the 22-byte empty archive.
 * Afterwards the ctx holds no index of either kind.
 * sfh_compress_zip_device_async: the host arrays and the names are read before the call returns; *d_out_n (device) = the
 * archive's bytes; the host does not wait for the stream (between two launch batches it waits, as the batch call does, for the
 * previous batch's descriptor tables to have gone up).  sfh_compress_zip_device synchronises and returns the size;
 * sfh_compress_zip takes host buffers, staged like sfh_compress_batch. */
size_t sfh_zip_bound(size_t count, const uint64_t* src_n, const uint32_t* name_len);
int sfh_compress_zip_device_async(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                  const char* const* names, const uint32_t* name_len, void* d_dst, size_t cap, uint64_t* d_out_n,
                                  const sfh_options* opt, void* stream);
int sfh_compress_zip_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, const char* const* names,
                            const uint32_t* name_len, void* d_dst, size_t cap, size_t* out_n, const sfh_options* opt, void* stream);
int sfh_compress_zip(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, const char* const* names,
                     const uint32_t* name_len, void* dst, size_t cap, size_t* out_n, const sfh_options* opt);

/* ---- decoding without side information ----
 * The segment index of a stream that is flushed every 32 KiB of output -- every stream sfh_compress* writes, and zlib's with
 * Z_SYNC_FLUSH / Z_FULL_FLUSH every 32768 input bytes -- recovered from the stream itself: a coded segment ends with the empty
 * stored block of a flush (bytes 00 00 FF FF), a stored segment is one block of LEN 32768.  One pass over the body finds both
 * patterns, pointer jumping walks them from the body's first byte.  container: enum sfh_container (the wrapper is read as
 * sfh_decompress_batch reads it).  Alignment as sfh_decompress_device (d_src 4, d_index 8, d_dst 16).
 *
 * sfh_recover_index_device: index[0..nseg] (nseg = max(1, ceil(dst_n / 32768)), offsets into the stream, wrapper header
 * included, as sfh_copy_index); d_depends (uint8 per segment, device, may be NULL): 1 when a match of the segment reaches
 * before its first byte (the token stage runs for it).  SFH_E_NOT_INDEXABLE when the walk ends short; a wrapper header that does
 * not parse is SFH_E_NOT_INDEXABLE as well.  Synchronises `stream` (NULL = the ctx's own).
 *
 * sfh_decompress_any_device: recovers the index and decodes with it: *status is the reference's DecompressStatus, and for a
 * wrapped stream container.hpp's decompress(src, dst, container) (header, ISIZE, the Adler-32 / CRC-32 computed on the GPU:
 * a mismatch is Error).  Every segment but the last must end exactly on its last byte with a non-final block, so Success means
 * the bytes the serial decoder writes; a false marker only ever ends in an error status.  No block_bytes: a match may reach
 * back as far as bytes were written, and segments are copied in rows of dependent segments found by the token stage.
 * dst_n = SFH_SIZE_FROM_TRAILER with a gzip stream: the output size is ISIZE (members of 4 GiB and more need an explicit size).
 * The token scratch is 4 bytes per output byte of the whole call.  Synchronises `stream`.
 * sfh_decompress_any: host buffers (H2D, the same, D2H of dst when *status is 0); dst holds dst_cap bytes (dst_n above it, or an
 * ISIZE above it, is SFH_E_DST_TOO_SMALL); *dst_n_out (may be NULL) = the output size decoded to.
 * Each of these calls runs as the batch call below with one item, and synchronises `stream` as that call does.  A stream of
 * more than 2^31 - 1 scan waves (8 KiB each: above 2^44 bytes) is SFH_E_INVALID_ARG. */
#define SFH_SIZE_FROM_TRAILER UINT64_MAX
int sfh_recover_index_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, uint64_t dst_n, uint64_t* d_index,
                             size_t nseg, uint8_t* d_depends, void* stream);
/* host buffers: index[0..nseg], depends (uint8 per segment, may be NULL) */
int sfh_recover_index(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, uint64_t dst_n, uint64_t* index, size_t nseg,
                      uint8_t* depends);
int sfh_decompress_any_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, void* d_dst, uint64_t dst_n,
                              uint32_t* status, void* stream);
int sfh_decompress_any(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, void* dst, uint64_t dst_cap,
                       uint64_t dst_n, uint64_t* dst_n_out, uint32_t* status);
/* Many block-flushed streams in one call, each with no side information and each decoded into its own buffer: what
 * sfh_compress_batch writes, read back with nothing but the streams.  For every item i, status[i], dst_n_out[i] and, on status
 * 0, the bytes are exactly what sfh_decompress_any_device gives for that item alone (container: the same for every item).  An
 * item for which the single call returns SFH_E_NOT_INDEXABLE gets status[i] = SFH_ITEM_NOT_INDEXABLE -- a per-item status,
 * never a DecompressStatus -- and its destination is not written; the call still returns SFH_OK (sfh_inflate_stream_batch*
 * decodes such items).  A wrapper that does not parse gives the item container.hpp's status, as in the single call.  One item's
 * failure or unindexability changes no other item's bytes or status, and nothing is written outside [dsts[i], dsts[i] +
 * dst_cap[i]).  dst_n[i]: the item's output size, or SFH_SIZE_FROM_TRAILER (gzip: ISIZE); a size or an ISIZE above dst_cap[i]
 * is DecompressStatus DstTooSmall (4) for that item, not a failure of the call.  dst_n_out (may be NULL) and status are host
 * arrays.
 * Refused with SFH_E_INVALID_ARG before anything is enqueued: a null ctx or an unknown container (also with count == 0); a null
 * array with count > 0, a null source with src_n > 0 or a null destination with dst_cap > 0; a device source not 4-byte, a
 * destination not 16-byte or the index not 8-byte aligned; a size above 2^44; SFH_SIZE_FROM_TRAILER with a container other
 * than gzip (or in a recover call); overlapping destination ranges; more than 2^31 - 1 segments or scan waves (8 KiB of an
 * item's stream each; an item of one segment has none) in the call.  count == 0 is SFH_OK.
 * Host synchronisations of `stream` (NULL = the ctx's own), per call and not per item: one after the wrappers (only when some
 * item's size is SFH_SIZE_FROM_TRAILER), one after the node count, one after the walk, one at the end of the decode.  The
 * recovery runs over the whole call (one scan, one walk over the items' node lists, each with its own end sentinel); the decode
 * in launch batches of whole items of at most SFH_BATCH_CHUNKS segments (a larger item alone and whole), so the token scratch is
 * that of the widest launch batch (sfh_last_decode_scratch_bytes).  sfh_last_recover_stats sums over the call,
 * sfh_last_inflate_ms over the launch batches.  Afterwards the ctx holds no index of either kind.
 * sfh_recover_index_batch_device: the walk alone.  d_index: flat, sfh_copy_batch_index's layout -- item i's max(1, ceil(dst_n[i]
 * / 32768)) + 1 entries behind those of the items before it; status[i] is 0 or SFH_ITEM_NOT_INDEXABLE (then the item's entries
 * are 0).
 * sfh_recover_index_batch, sfh_decompress_any_batch: host buffers, packed through the pinned staging; only items whose status
 * is 0 are copied back. */
#define SFH_ITEM_NOT_INDEXABLE 0xFFFFFFF8u /* (uint32_t)SFH_E_NOT_INDEXABLE */
int sfh_recover_index_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                                   const uint64_t* dst_n, uint64_t* d_index, uint32_t* status, void* stream);
int sfh_decompress_any_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n, uint32_t container,
                                    void* const* d_dsts, const uint64_t* dst_cap, const uint64_t* dst_n, uint64_t* dst_n_out,
                                    uint32_t* status, void* stream);
int sfh_recover_index_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                            const uint64_t* dst_n, uint64_t* index, uint32_t* status);
int sfh_decompress_any_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n, uint32_t container,
                             void* const* dsts, const uint64_t* dst_cap, const uint64_t* dst_n, uint64_t* dst_n_out,
                             uint32_t* status);
/* the last sfh_recover_index* / sfh_decompress_any* call: ms[0] candidate scan, ms[1] walk (with profiling on, else zeros);
 * counts[0] nodes (b0, markers, stored headers), counts[1] rows of dependent segments (0 when no decode ran) */
int sfh_last_recover_stats(sfh_ctx* ctx, float ms[2], uint64_t counts[2]);

/* One raw, zlib or gzip stream (one member) with no side information and no flush points, decoded on the GPU (DESIGN.md 3a,
 * "Streams without flush points").  The body is cut at speculative dynamic-block starts every SFH_STREAM_CHUNK bytes (default
 * 16384; the environment at sfh_create), the chunks are decoded lane-serially and chained: a chunk counts only when the chunk
 * before it ends, without BFINAL, exactly on its start, so a wrong guess costs time and never changes a byte or a status.
 * *status is what container.hpp's decompress(src, dst, container) returns for a dst of dst_cap bytes (raw: decompress(src,
 * dst)), the first problem in stream order; *dst_n_out the bytes the body produced (on Success: dst[0, *dst_n_out) is the
 * output).  One difference, on purpose: container.hpp takes a zlib dst to be exactly the output size and checks the Adler-32
 * over all of it, so a larger dst is Error there; here the output size need not be known, and the Adler-32 is checked over the
 * bytes produced (zlib's own rule) -- with dst_cap equal to the output size both agree.  Candidate block starts are
 * dynamic-Huffman headers and, inside a run of stored blocks, non-final stored-block headers with zero padding bits, so a
 * stream of stored blocks (level 0, or data zlib could not compress) is cut at its blocks; the last block of a run is not a
 * cut.  Fixed-Huffman blocks are no candidates: a Z_FIXED stream is decoded
 * by one lane: slow, but correct.
 * Size query: d_dst == NULL and dst_cap == 0 runs the candidate, count and chain steps only: *dst_n_out = the output size, and
 * *status the wrapper's or the first structural problem of the body (the checks that need output positions -- distance <=
 * bytes written, the capacity, the checksum -- are the decode call's).
 * The call is the batched call below with one item: one decoder runs both.  d_src 4-byte aligned, d_dst 16-byte aligned.  A
 * call on another stream than the ctx's previous call first waits, on the device, for that call (raw streams included: the
 * calls share the ctx's scratch).  Host synchronisations of `stream` (NULL = the ctx's own): the wrapper (zlib and gzip; a raw
 * stream has none), the candidates, the count pass and each chain round, the write pass's statuses, and one at the end of the
 * decode (with a wrapper: behind the checksum).  Scratch: 60 bytes per nominal chunk, 2 bytes per output byte (the symbol
 * plane, rounded up to 16 entries, 16 bytes at least) and 64 KiB per group of about sqrt(chunks) chunks beyond the first
 * (sfh_last_decode_scratch_bytes; the size query: the first term only).  After a non-zero *status sfh_last_error reads
 * "DecompressStatus N".
 * sfh_inflate_stream: host buffers (H2D, the same, D2H of dst when *status is 0); dst == NULL with dst_cap == 0 is the size query.
 *
 * Files of gzip members (container = SFH_GZIP_MEMBERS; these four calls only).  src is a series of gzip members, each with its
 * own header, body, CRC-32 and ISIZE, zero bytes allowed behind every trailer (tape padding, as gzip and Python skip it).
 * *status and *dst_n_out are what container.hpp's decompress_members(src, dst[dst_cap]) -- its Container::GzipMembers case --
 * gives: every member decodes behind the one before it, dst may be larger than the output, a member has no history (a match
 * that reaches before its member's first byte is InvalidDistance), output beyond dst_cap is DstTooSmall, an empty src, a
 * trailer of fewer than 8 bytes or fewer than 18 bytes behind the zero bytes are SrcTooSmall, anything else that is no gzip
 * header behind a trailer is Error, and so is an ISIZE (modulo 2^32) or a CRC-32 that does not match its member's own output.
 * Empty members count.  After a non-zero *status *dst_n_out is not specified.
 * ONE DIFFERENCE from the host function: it checks a member's trailer before it reads the next member; here the trailers'
 * values are checked after every body of the item has decoded.  A file in which one member's CRC-32 or ISIZE is wrong AND a
 * later member's header or body is faulty has the later fault's status here and Error there; both are non-zero.
 * The size query returns the total output size and the first structural problem -- a bad header behind a trailer or a short
 * trailer included --; ISIZE and CRC-32 values are the decode call's to check.
 * The file is decoded as one stream: where a member ends, the decoding lane steps over trailer, padding and header and goes on,
 * and the start of a member's body is a chunk candidate as well, so a file of many small members is cut as finely as one large
 * stream.  Scratch: 16 bytes per candidate and 32 bytes per member more; the checksums run per member, all members of a
 * launch batch in one launch, and the call has one host synchronisation more than above (the chunks' member counts, behind
 * the chain rounds), however many members there are.  More than 2^31 - 1 members in a call: SFH_E_INVALID_ARG once the count pass knows, before any
 * byte is written.  A member whose output is 4 GiB or more is not supported (its checksum is not folded correctly).
 * Which reader for which file: INTEGRATION.md. */
int sfh_inflate_stream_device(sfh_ctx* ctx, const void* d_src, size_t src_n, uint32_t container, void* d_dst, uint64_t dst_cap,
                              uint64_t* dst_n_out, uint32_t* status, void* stream);
int sfh_inflate_stream(sfh_ctx* ctx, const void* src, size_t src_n, uint32_t container, void* dst, uint64_t dst_cap,
                       uint64_t* dst_n_out, uint32_t* status);
/* Many such streams in one call, each decoded into its own buffer.  For every item i, status[i], dst_n_out[i] and, on status 0,
 * the bytes dsts[i][0, dst_n_out[i]) are exactly what sfh_inflate_stream_device returns for that item alone with dst_cap[i]
 * (container: the same for every item).  One item's failure changes no other item's bytes or status; nothing is written
 * outside [dsts[i], dsts[i] + dst_cap[i]), and an item's destination only on its status 0 (or after a checksum mismatch).
 * dst_n_out and status are host arrays; the call synchronises `stream` (NULL = the ctx's own).  Size query: d_dsts == NULL
 * (dst_cap may then be NULL) runs the candidate, count and chain steps for every item; an item whose dsts[i] is NULL is a size
 * query of its own.  Refused with SFH_E_INVALID_ARG before anything is enqueued: a null ctx or an unknown container (also with
 * count == 0); a null array with count > 0, or a null source with src_n > 0 (a null destination with dst_cap > 0); a device
 * source not 4-byte or destination not 16-byte aligned; dst_cap above 2^44; overlapping destination ranges (an empty one
 * overlaps nothing); more than 2^31 - 1 nominal chunks (ceil(src_n / SFH_STREAM_CHUNK), at least 1 per item) in the call.
 * count == 0 is SFH_OK.  The candidate, count and chain steps run over the whole call; the write pass, the windows and the
 * checksums in launch batches of whole items of at most SFH_BATCH_CHUNKS * 32 KiB of output (1 GiB by default; a larger item
 * alone).  Host synchronisations: the wrapper, the candidates, each chain round (the most any item needs), and per launch batch
 * the statuses and the checksums -- not more with more items.  Scratch: 60 bytes per nominal chunk of the call, and per launch
 * batch 2 bytes per output byte and 64 KiB per group (sfh_last_decode_scratch_bytes: the peak).  sfh_last_stream_stats: counts
 * [0] to [2] summed over the items, [3] and [4] their maxima, [5] the peak scratch; stage times summed.
 * sfh_inflate_stream_batch: host buffers, packed through pinned staging (one copy per direction per 64 MiB); only items whose
 * status is 0 are copied back. */
int sfh_inflate_stream_batch_device(sfh_ctx* ctx, size_t count, const void* const* d_srcs, const uint64_t* src_n,
                                    uint32_t container, void* const* d_dsts, const uint64_t* dst_cap,
                                    uint64_t* dst_n_out, uint32_t* status, void* stream);
int sfh_inflate_stream_batch(sfh_ctx* ctx, size_t count, const void* const* srcs, const uint64_t* src_n,
                             uint32_t container, void* const* dsts, const uint64_t* dst_cap,
                             uint64_t* dst_n_out, uint32_t* status);
/* the last sfh_inflate_stream* call (a batch call: see above).  ms (profiling on, else zeros): SFH_STREAM_NSTAGES stages -- find, count (the first count
 * pass and every repair round), write, resolve, checksum.  counts: [0] nominal chunks, [1] candidates (chunk 0 included), [2]
 * confirmed chunks, [3] repair rounds, [4] the longest confirmed chunk's output bytes, [5] scratch bytes */
#define SFH_STREAM_NSTAGES 5
#define SFH_STREAM_NCOUNTS 6
int sfh_last_stream_stats(sfh_ctx* ctx, float ms[SFH_STREAM_NSTAGES], uint64_t counts[SFH_STREAM_NCOUNTS]);

/* bytes of decoder token scratch the last sfh_decompress* call on this ctx used (0 before the first) */
size_t sfh_last_decode_scratch_bytes(const sfh_ctx* ctx);

#define SFH_INFLATE_NSTAGES 2 /* 0 k_inflate_tokens (Huffman decode), 1 k_inflate_bytes (match copies) */
/* with profiling on: milliseconds per decoder kernel of the last sfh_decompress* call (summed over its batches) */
int sfh_last_inflate_ms(sfh_ctx* ctx, float ms[SFH_INFLATE_NSTAGES]);
const char* sfh_inflate_stage_name(int stage);

/* ---- container checksums ---- */

/* Checksum of n device bytes (d_src 16-byte aligned): kind = SFH_ZLIB -> Adler-32, SFH_GZIP -> CRC-32,
 * bit-exact with zlib's adler32()/crc32().  Synchronises `stream` (NULL = the ctx's own). */
int sfh_checksum_device(sfh_ctx* ctx, const void* d_src, size_t n, uint32_t kind, uint32_t* out, void* stream);
/* Checksum of A||B from the checksums of A and B and the length of B (host arithmetic; a multi-GPU job
 * combines its shards' checksums with these and writes one wrapper around the concatenated raw streams). */
uint32_t sfh_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint32_t sfh_adler32_combine(uint32_t adler_a, uint32_t adler_b, uint64_t len_b);

#define SFH_NSTAGES 5 /* 0 lz77 match+parse, 1 code plan, 2 offset scan, 3 emit, 4 checksum + wrapper (container modes) */

/* on != 0: bracket every kernel launch with HIP events on the launch stream */
void sfh_set_profiling(sfh_ctx* ctx, int on);
/* after the stream has been synchronised: milliseconds per stage of the last call */
int sfh_last_stage_ms(sfh_ctx* ctx, float ms[SFH_NSTAGES]);
const char* sfh_stage_name(int stage);

/* ---- stage inspection for parity tests: copies device scratch of the last call ---- */
enum sfh_debug_what {
  SFH_DBG_NTOK = 0,   /* uint32 per chunk */
  SFH_DBG_TOKENS = 1, /* decoder: uint32[32768] per segment, first ntok valid */
  SFH_DBG_ITEMS = 8,  /* compressor: uint16[32768] per chunk, first nitems valid (literal: 0x8000 | byte; match: 0x8100 | len-3,
                         then dist-1 with bit 15 clear; 0x4000 + region index in bits 9..13 on a parse region's first item) */
  SFH_DBG_NITEMS = 9, /* uint32 per chunk */
  SFH_DBG_HIST = 2,   /* uint32[576] per chunk: ll[0..285], d at [288..317], raw len-3 counts at [320..575] */
  SFH_DBG_PLAN = 3,   /* uint32[4] per chunk: btype, out_bytes, header_bits, body_bits */
  SFH_DBG_LENS = 4,   /* uint8[320] per chunk: ll lens [0..287], d lens [288..319] */
  SFH_DBG_OFFSETS = 5, /* uint64 per chunk */
  SFH_DBG_SUBINDEX = 7, /* uint32[64] per chunk */
  SFH_DBG_SEGINFO = 10, /* decoder: uint32[6] per segment {status, tokens, bit 0 stored segment | bit 1 decoded by the
                           lane-serial kernel, bytes, offset of a stored segment's bytes (u64)} */
  SFH_DBG_RITEM = 11, /* compressor: uint32[32] per chunk, the item index of each 1024-byte region's first token (regions
                         past the data: nitems) */
  SFH_DBG_STAMPS = 6,  /* uint64[2][nchunks][8] (k_lz77, k_plan); only with env SFH_K1_STAMPS=1 at sfh_create
                          (diagnostic k_lz77 build: cycles per phase, never a timing claim) */
  SFH_DBG_STREAM_MEMBERS = 12 /* the member table of the last call when that was an sfh_inflate_stream* call with SFH_GZIP_MEMBERS
                          (after any other call: SFH_E_INVALID_ARG): uint64 count, then count records of 32 bytes {uint64 src_end
                          (the offset just past the member's trailer), uint64 out_end, uint32 crc32, uint32 isize (the trailer's
                          values), uint32 item, uint32 status (0, or 1: the trailer does not match the member's output)}.  Offsets
                          are relative to the item; records in call order, an item's members in file order; only items whose
                          bodies decoded have records (a size query has none).  bytes >= 8: the count, and as many whole records
                          as fit */
};
int sfh_debug_read(sfh_ctx* ctx, int what, void* host_dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
