// starflate::compress -- the sibling of decompress(): raw RFC 1951 (optionally zlib / gzip wrapped) out of
// the MI355X kernels.
// Thin C++23 wrapper over the C-ABI (include/starflate_hip.h); link with libstarflate_hip.so.
// Same conventions as the reference's one public function
// (/root/reference/src/decompress.hpp:63-71): non-owning spans, caller-owned buffers, no
// exceptions, a uint8_t status enum; the size comes back through expected<>.
#pragma once
#include "starflate/compat/expected.hpp"
#include "starflate/container.hpp"
#include "starflate_hip.h"

#include <cstddef>
#include <cstdint>
#include <span>
#include <string_view>
#include <utility>
#include <vector>

namespace starflate {

enum class CompressStatus : std::uint8_t {
  Success,
  InvalidArgument,
  DstTooSmall,  // dst.size() < compress_bound(src.size())
  NoDevice,     // no MI355X visible: there is no CPU fallback
  DeviceError,
  OutOfMemory,
  CommError,    // RCCL not loadable, or an RCCL call failed (gather_streams)
  Unsupported,  // the effort rests on LDS behaviour this device does not show (sfh_lds_order_check)
  NotIndexable, // recover_index: the stream is not block-flushed every 32 KiB of output
};

enum class BlockStrategy : std::uint8_t { Auto, Stored, Fixed, Dynamic };

/// How hard the match finder looks (== enum sfh_effort of the C-ABI, value for value).
///   Default : every other position searched, two history levels per hash bucket + the step-local candidate
///   Fast    : the newer history level only, about 3 % more output
///   Fastest : that, and no step-local candidate
///   Thorough: every position searched
///   Max     : Thorough with a second hash table keyed by seven bytes
///   Best / Ultra / Extreme: exact hash chains of depth 8 / 16 / 32 (zlib's structure) instead of the step tables
///   Recent / RecentAll: the step tables with EXACT RECENCY -- a bucket holds the latest position with the hash and the one
///             before the latest inserting step, a position's nearest earlier occurrence is its third candidate; every
///             other position searched (Recent: DEPRECATED -- Thorough's ratio at Thorough's speed on every workload
///             measured, kept for compatibility) or every position (RecentAll: the effort for real source text / machine code)
enum class Effort : std::uint8_t {
  Default = SFH_EFFORT_DEFAULT,
  Fast = SFH_EFFORT_FAST,
  Fastest = SFH_EFFORT_FASTEST,
  Thorough = SFH_EFFORT_THOROUGH,
  Max = SFH_EFFORT_MAX,
  Best = SFH_EFFORT_BEST,    // exact hash chains, the 8 most recent positions with the hash
  Ultra = SFH_EFFORT_ULTRA,  // ... the 16 most recent
  Extreme = SFH_EFFORT_EXTREME,  // ... the 32 most recent: zlib -6's own ratio
  Recent [[deprecated("no point of its own on the speed / ratio curve: use Thorough or RecentAll")]] = SFH_EFFORT_RECENT,
  RecentAll = SFH_EFFORT_RECENT_ALL,
};

struct compress_options {
  BlockStrategy strategy{BlockStrategy::Auto};
  bool final_stream{true};  // false: byte-aligned, non-final stream (a shard that is not the last)
  std::uint8_t lazy{3};     // 0..3 positions of look-ahead of the lazy match rule (sfh_options.lazy)
  bool stored_fast_path{true};  // skip the search of a chunk whose first 8 KiB are (almost) all literals
  Container container{Container::Raw};  // Zlib / Gzip: wrapper + GPU-computed Adler-32 / CRC-32 (needs final_stream);
                                        // Dictzip: Gzip with the random-access table in its header (block_bytes 0 or 32768,
                                        // at most SFH_DZ_MAX_CHUNKS * 32768 bytes; compressor::compress and compress_device* only)
  int device{0};
  Effort effort{Effort::Default};  // sfh_options.effort
  std::uint8_t chain_depth{0};     // sfh_options.chain_depth: with Best / Ultra / Extreme, candidates per position (0: 8 / 16 / 32)
  std::uint32_t block_bytes{0};  // bytes coded independently of what precedes them: a multiple of 32768, 0 = default
                                 // (sfh_options.block_bytes); larger compresses better, 32768 = independent DEFLATE blocks
};

inline auto compress_bound(std::size_t n, std::uint32_t block_bytes = 0) -> std::size_t { return sfh_compress_bound(n, block_bytes); }
/// ... for a container: Container::Dictzip's header carries two bytes per 32 KiB of input (0: what the call would refuse)
inline auto compress_bound(std::size_t n, std::uint32_t block_bytes, Container container) -> std::size_t {
  return sfh_compress_bound_container(n, block_bytes, static_cast<std::uint32_t>(container));
}

/// What makes a stream of this library decodable in parallel (on the GPU): the first stream byte of every
/// 32 KiB segment plus the end of the last one, the strip size (no match reaches before its strip), and
/// optionally, per segment, 32 x {bit offset of the first token code of every 1024 bytes, tokens before it}.
/// Side information: the stream itself is plain DEFLATE.
struct stream_index {
  std::vector<std::uint64_t> offsets;  // segments + 1
  std::vector<std::uint32_t> regions;  // segments * 64, or empty
  std::uint32_t block_bytes{SFH_SEGMENT_BYTES};  // strip size the stream was written with
  std::uint64_t total_bytes{0};        // the stream's whole output size: filled by compressor::index() and recover_index(),
                                       // read by decompress_range[s] (segments() == max(1, ceil(total_bytes / 32768)))
  [[nodiscard]] auto segments() const -> std::size_t { return offsets.empty() ? 0 : offsets.size() - 1; }
};

/// The index of a compress batch (compressor::batch_index): every item's stream_index, flattened item after item.  Item i's
/// segments + 1 offsets (relative to its own stream) are offsets[first[i] .. first[i + 1]), its sub-index words
/// regions[64 * (first[i] - i) ..) (64 per segment; empty: none), its strip size block_bytes[i].
struct batch_stream_index {
  std::vector<std::uint64_t> offsets;
  std::vector<std::uint32_t> regions;
  std::vector<std::uint32_t> block_bytes;
  std::vector<std::size_t> first;  // items + 1
  [[nodiscard]] auto items() const -> std::size_t { return block_bytes.size(); }
};

namespace detail {
inline auto to_status(int rc) -> CompressStatus {
  switch (rc) {
    case SFH_OK: return CompressStatus::Success;
    case SFH_E_DST_TOO_SMALL: return CompressStatus::DstTooSmall;
    case SFH_E_NO_DEVICE: return CompressStatus::NoDevice;
    case SFH_E_HIP: return CompressStatus::DeviceError;
    case SFH_E_NOMEM: return CompressStatus::OutOfMemory;
    case SFH_E_COMM: return CompressStatus::CommError;
    case SFH_E_UNSUPPORTED: return CompressStatus::Unsupported;
    case SFH_E_NOT_INDEXABLE: return CompressStatus::NotIndexable;
    default: return CompressStatus::InvalidArgument;
  }
}
/// what the decoders' `container` argument takes: to them a dictzip file is a gzip stream
static_assert(static_cast<std::uint32_t>(Container::GzipMembers) == SFH_GZIP_MEMBERS);  // (the stream decoders only)
inline auto to_c(Container c) -> std::uint32_t { return c == Container::Dictzip ? SFH_GZIP : static_cast<std::uint32_t>(c); }
inline auto to_c(const compress_options& o) -> sfh_options {
  sfh_options c;
  sfh_default_options(&c);
  c.strategy = static_cast<std::uint32_t>(o.strategy);
  c.final_stream = o.final_stream ? 1U : 0U;
  c.lazy = o.lazy;
  c.no_stored_fast_path = o.stored_fast_path ? 0U : 1U;
  c.container = static_cast<std::uint32_t>(o.container);
  c.block_bytes = o.block_bytes;
  c.effort = static_cast<std::uint32_t>(o.effort);
  c.chain_depth = o.chain_depth;
  return c;
}
}  // namespace detail

/// The index a dictzip file of 32 KiB chunks carries in its own header (sfh_dz_read_index: host arithmetic, no device):
/// offsets, block_bytes 32768 and total_bytes (ISIZE), what compressor::decompress_range[s] and decompress() take.  A gzip file
/// without such a table is CompressStatus::NotIndexable, a header that does not parse InvalidArgument.
inline auto dz_read_index(std::span<const std::byte> src) -> compat::expected<stream_index, CompressStatus> {
  stream_index ix;
  ix.offsets.resize(static_cast<std::size_t>(SFH_DZ_MAX_CHUNKS) + 1);
  sfh_dz_info info{};
  const int rc = sfh_dz_read_index(src.data(), src.size(), &info, ix.offsets.data(), ix.offsets.size());
  if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
  if (info.status != 0) return compat::unexpected{CompressStatus::InvalidArgument};
  ix.offsets.resize(static_cast<std::size_t>(info.nseg) + 1);
  ix.block_bytes = SFH_SEGMENT_BYTES;
  ix.total_bytes = info.total_n;
  return ix;
}

/// BGZF, the blocked gzip of bgzip / htslib (sfh_compress_bgzf*, sfh_bgzf_read_index*, sfh_decompress_bgzf*): the capacity
/// compressor::compress_bgzf needs for n input bytes ...
inline auto bgzf_bound(std::size_t n) -> std::size_t { return sfh_bgzf_bound(n); }
/// ... and the members of such a file, found on the host (no device): every member's first byte and the file's size, the prefix
/// sums of the members' ISIZE, and what sfh_bgzf_info says.  A file that does not parse is InvalidArgument.
struct bgzf_index {
  std::vector<std::uint64_t> member_off;  // members + 1
  std::vector<std::uint64_t> out_off;     // members + 1; out_off.back() == total_bytes
  std::uint64_t total_bytes{0};
  std::uint32_t max_isize{0};
  bool has_eof{false};
  [[nodiscard]] auto members() const -> std::size_t { return member_off.empty() ? 0 : member_off.size() - 1; }
};
inline auto bgzf_read_index(std::span<const std::byte> src) -> compat::expected<bgzf_index, CompressStatus> {
  sfh_bgzf_info info{};
  (void)sfh_bgzf_read_index(src.data(), src.size(), &info, nullptr, nullptr, 0);  // the count (SFH_E_DST_TOO_SMALL: it is there)
  if (info.status != 0) return compat::unexpected{CompressStatus::InvalidArgument};
  bgzf_index ix;
  ix.member_off.resize(static_cast<std::size_t>(info.members) + 1);
  ix.out_off.resize(static_cast<std::size_t>(info.members) + 1);
  const int rc = sfh_bgzf_read_index(src.data(), src.size(), &info, ix.member_off.data(), ix.out_off.data(), ix.member_off.size());
  if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
  ix.total_bytes = info.total_n;
  ix.max_isize = info.max_isize;
  ix.has_eof = info.has_eof != 0;
  return ix;
}
/// Virtual offsets, as tabix and BAI indexes state them (coffset << 16 | uoffset), to offsets into the file's output and back
/// (sfh_bgzf_voffsets_to_offsets, sfh_bgzf_offsets_to_voffsets: host arithmetic).  A virtual offset that names no member's first
/// byte, or a byte behind its output, and an offset above total_bytes give UINT64_MAX in their slot.
inline auto bgzf_voffsets_to_offsets(const bgzf_index& ix, std::span<const std::uint64_t> voffsets) -> std::vector<std::uint64_t> {
  std::vector<std::uint64_t> out(voffsets.size(), ~std::uint64_t{0});
  if (ix.member_off.empty() || ix.out_off.size() != ix.member_off.size()) return out;
  (void)sfh_bgzf_voffsets_to_offsets(ix.member_off.data(), ix.out_off.data(), static_cast<std::uint32_t>(ix.members()), out.size(),
                                     voffsets.data(), out.data());
  return out;
}
inline auto bgzf_offsets_to_voffsets(const bgzf_index& ix, std::span<const std::uint64_t> offsets) -> std::vector<std::uint64_t> {
  std::vector<std::uint64_t> out(offsets.size(), ~std::uint64_t{0});
  if (ix.member_off.empty() || ix.out_off.size() != ix.member_off.size()) return out;
  (void)sfh_bgzf_offsets_to_voffsets(ix.member_off.data(), ix.out_off.data(), static_cast<std::uint32_t>(ix.members()), out.size(),
                                     offsets.data(), out.data());
  return out;
}

/// ZIP archives (sfh_zip_read_index*, sfh_decompress_zip*, sfh_compress_zip*): the capacity compressor::compress_zip needs for
/// items of these sizes under names of these lengths ...
inline auto zip_bound(std::span<const std::uint64_t> sizes, std::span<const std::uint32_t> name_lens) -> std::size_t {
  return sizes.size() == name_lens.size() ? sfh_zip_bound(sizes.size(), sizes.data(), name_lens.data()) : 0;
}
/// ... and the entry table of an archive in host memory (no device): sfh_zip_entry rows -- where every entry's data lies, its
/// sizes, CRC-32, method and its own status (0, a DecompressStatus, or SFH_ZIP_ENTRY_UNSUPPORTED) -- and what sfh_zip_info
/// says.  name(file, i): entry i's name, read where the table says it stands in the file.  An archive whose end record or
/// directory does not parse is InvalidArgument.
struct zip_index {
  std::vector<sfh_zip_entry> entries;
  std::uint64_t total_out{0};  // the packed layout's bytes: every entry at entries[i].out_off, 16-byte aligned
  bool zip64{false};
  [[nodiscard]] auto name(std::span<const std::byte> file, std::size_t i) const -> std::string_view {
    const auto& e = entries[i];
    if (e.name_off > file.size() || file.size() - e.name_off < e.name_len) return {};
    return {reinterpret_cast<const char*>(file.data()) + e.name_off, e.name_len};
  }
};
inline auto zip_read_index(std::span<const std::byte> file) -> compat::expected<zip_index, CompressStatus> {
  sfh_zip_info info{};
  (void)sfh_zip_read_index(file.data(), file.size(), &info, nullptr, 0);  // the count (SFH_E_DST_TOO_SMALL: it is there)
  if (info.status != 0) return compat::unexpected{CompressStatus::InvalidArgument};
  zip_index ix;
  ix.entries.resize(static_cast<std::size_t>(info.entries));
  const int rc = sfh_zip_read_index(file.data(), file.size(), &info, ix.entries.data(), ix.entries.size());
  if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
  ix.total_out = info.total_out;
  ix.zip64 = info.zip64 != 0;
  return ix;
}

/// One GPU context (device scratch, stream).  Not thread-safe; distinct objects are independent.
class compressor {
  sfh_ctx* ctx_{nullptr};
  CompressStatus init_{CompressStatus::Success};
  std::vector<std::uint64_t> batch_n_;  // the items' sizes of the last compress_batch() (what batch_index() cuts the index by)
  std::uint64_t last_n_{0};             // the input size of the last single compress call (index().total_bytes)

 public:
  explicit compressor(int device = 0) { init_ = detail::to_status(sfh_create(&ctx_, device)); }
  compressor(const compressor&) = delete;
  auto operator=(const compressor&) -> compressor& = delete;
  compressor(compressor&& o) noexcept : ctx_{std::exchange(o.ctx_, nullptr)}, init_{o.init_}, batch_n_{std::move(o.batch_n_)}, last_n_{o.last_n_} {}
  auto operator=(compressor&& o) noexcept -> compressor& {
    if (this != &o) {
      sfh_destroy(ctx_);
      ctx_ = std::exchange(o.ctx_, nullptr);
      init_ = o.init_;
      batch_n_ = std::move(o.batch_n_);
      last_n_ = o.last_n_;
    }
    return *this;
  }
  ~compressor() { sfh_destroy(ctx_); }
  [[nodiscard]] auto status() const -> CompressStatus { return init_; }
  [[nodiscard]] auto native() const -> sfh_ctx* { return ctx_; }  // for the C-ABI entry points taking several contexts

  /// host spans: H2D, compress, D2H
  auto compress(std::span<const std::byte> src, std::span<std::byte> dst, const compress_options& opt = {})
      -> compat::expected<std::size_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    const auto c = detail::to_c(opt);
    std::size_t n = 0;
    const int rc = sfh_compress(ctx_, src.data(), src.size(), dst.data(), dst.size(), &n, &c);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    last_n_ = src.size();
    return n;
  }
  /// host spans: a BGZF file -- one gzip member per 32768 input bytes, then the EOF member -- that bgzip -d and htslib read
  /// (sfh_compress_bgzf).  dst.size() >= bgzf_bound(src.size()); opt.container must be Raw (the call is the wrapper),
  /// final_stream true, block_bytes 0 or 32768.  The context holds no index afterwards.
  auto compress_bgzf(std::span<const std::byte> src, std::span<std::byte> dst, const compress_options& opt = {})
      -> compat::expected<std::size_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    const auto c = detail::to_c(opt);
    std::size_t n = 0;
    const int rc = sfh_compress_bgzf(ctx_, src.data(), src.size(), dst.data(), dst.size(), &n, &c);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    return n;
  }
  /// A BGZF file decoded (sfh_decompress_bgzf: members of any size; every member's header, ISIZE and CRC-32 verified).
  /// dst.size() >= the members' ISIZEs together (bgzf_read_index); *produced (nullable) = that sum on Success.  A refused call
  /// or a device problem is Error.  Every conforming file decodes in the indexed decoder: members of at most 32768 bytes in
  /// its narrow rows, a file with a member of up to 65536 bytes (bgzip and htslib write 65280) in its wide rows.  For device
  /// buffers call sfh_decompress_bgzf_wide_device(native(), ...) -- it reads every conforming file -- or, for files of
  /// 32 KiB members only, sfh_decompress_bgzf_device (starflate_hip.h).
  auto decompress_bgzf(std::span<const std::byte> src, std::span<std::byte> dst, std::size_t* produced = nullptr) -> DecompressStatus {
    if (!ctx_) return DecompressStatus::Error;
    std::uint32_t st = 0;
    std::uint64_t n = 0;
    const int rc = sfh_decompress_bgzf(ctx_, src.data(), src.size(), dst.data(), dst.size(), &n, &st);
    if (rc == SFH_E_DST_TOO_SMALL) return DecompressStatus::DstTooSmall;
    if (rc != SFH_OK || st > 7) return DecompressStatus::Error;
    if (st == 0 && produced != nullptr) *produced = static_cast<std::size_t>(n);
    return static_cast<DecompressStatus>(st);
  }
  /// host spans: one ZIP archive of deflated entries, item i under names[i] (UTF-8, 1 to 65535 bytes), that unzip and zipfile
  /// read (sfh_compress_zip).  dst.size() >= zip_bound(...); opt.container must be Raw and final_stream true.  Every entry's
  /// body is byte for byte what compress_batch writes for that item with the same options.  No index afterwards.
  auto compress_zip(std::span<const std::string_view> names, std::span<const std::span<const std::byte>> srcs,
                    std::span<std::byte> dst, const compress_options& opt = {}) -> compat::expected<std::size_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    if (names.size() != srcs.size()) return compat::unexpected{CompressStatus::InvalidArgument};
    const std::size_t k = srcs.size();
    std::vector<const void*> sp(k);
    std::vector<const char*> np(k);
    std::vector<std::uint64_t> sn(k);
    std::vector<std::uint32_t> nl(k);
    for (std::size_t i = 0; i < k; ++i) {
      sp[i] = srcs[i].data();
      sn[i] = srcs[i].size();
      np[i] = names[i].data();
      nl[i] = names[i].size() > 65535 ? 65536U : static_cast<std::uint32_t>(names[i].size());  // (above the limit: refused)
    }
    const auto c = detail::to_c(opt);
    std::size_t n = 0;
    const int rc = sfh_compress_zip(ctx_, k, sp.data(), sn.data(), np.data(), nl.data(), dst.data(), dst.size(), &n, &c);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    return n;
  }
  /// Entries of a ZIP archive decoded (sfh_decompress_zip): entries[i] -- rows of zip_read_index(file), any subset in any order
  /// -- into dsts[i] (dsts[i].size() >= its usize); statuses[i] = 0, the entry's DecompressStatus (a CRC-32 mismatch is 1), or
  /// the status the index gave it (SFH_ZIP_ENTRY_UNSUPPORTED among them).  Only entries with status 0 are written.
  auto decompress_zip(std::span<const std::byte> file, std::span<const sfh_zip_entry> entries, std::span<const std::span<std::byte>> dsts,
                      std::span<std::uint32_t> statuses) -> CompressStatus {
    if (!ctx_) return init_;
    if (dsts.size() != entries.size() || statuses.size() != entries.size()) return CompressStatus::InvalidArgument;
    const std::size_t k = entries.size();
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> dn(k);
    for (std::size_t i = 0; i < k; ++i) {
      dp[i] = dsts[i].data();
      dn[i] = dsts[i].size();
    }
    return detail::to_status(sfh_decompress_zip(ctx_, file.data(), file.size(), entries.data(), k, dp.data(), dn.data(), statuses.data()));
  }
  /// host spans, many independent items in one call: item i's stream goes to dsts[i] (dsts[i].size() >=
  /// compress_bound(srcs[i].size())), its size to sizes[i]; byte-identical to compress(srcs[i], dsts[i], opt).
  /// Returns the bytes of all streams together.
  auto compress_batch(std::span<const std::span<const std::byte>> srcs, std::span<const std::span<std::byte>> dsts,
                      std::span<std::size_t> sizes, const compress_options& opt = {})
      -> compat::expected<std::size_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    if (dsts.size() != srcs.size() || sizes.size() != srcs.size()) return compat::unexpected{CompressStatus::InvalidArgument};
    const std::size_t k = srcs.size();
    std::vector<const void*> sp(k);
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> n(k), cap(k), out(k);
    for (std::size_t i = 0; i < k; ++i) {
      sp[i] = srcs[i].data();
      n[i] = srcs[i].size();
      dp[i] = dsts[i].data();
      cap[i] = dsts[i].size();
    }
    const auto c = detail::to_c(opt);
    const int rc = sfh_compress_batch(ctx_, k, sp.data(), n.data(), dp.data(), cap.data(), out.data(), &c);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    batch_n_ = std::move(n);
    std::size_t total = 0;
    for (std::size_t i = 0; i < k; ++i) total += sizes[i] = static_cast<std::size_t>(out[i]);
    return total;
  }
  /// index of the last call on this object when it was compress_batch() (with_regions: also the sub-index)
  auto batch_index(bool with_regions = true) -> compat::expected<batch_stream_index, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    std::size_t k = 0, entries = 0;
    if (sfh_batch_index_size(ctx_, &k, &entries) != SFH_OK || k != batch_n_.size())
      return compat::unexpected{CompressStatus::InvalidArgument};
    batch_stream_index ix;
    ix.offsets.resize(entries);
    ix.block_bytes.resize(k);
    ix.first.resize(k + 1);
    for (std::size_t i = 0; i < k; ++i)
      ix.first[i + 1] = ix.first[i] + static_cast<std::size_t>(batch_n_[i] ? (batch_n_[i] + SFH_SEGMENT_BYTES - 1) / SFH_SEGMENT_BYTES : 1) + 1;
    if (with_regions) ix.regions.resize((entries - k) * SFH_SUBINDEX_WORDS);
    const int rc = sfh_copy_batch_index(ctx_, ix.offsets.data(), with_regions ? ix.regions.data() : nullptr, ix.block_bytes.data(), 0, nullptr);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    return ix;
  }
  /// Many independent streams decoded in one call: srcs[i] into exactly dsts[i].size() bytes at dsts[i], its status into
  /// statuses[i] -- a raw item's what decompress(src, dst, ix) gives on it alone, a wrapped one's what
  /// decompress(srcs[i], dsts[i], container) (container.hpp) gives.  ix: batch_index() of the compress_batch() that wrote
  /// the streams (or any index of that layout); nullptr when every dsts[i].size() <= 32768 (each stream one segment: pages
  /// from other tools).  dsts[i] is written only where statuses[i] is Success.  A refused call (arguments, no device) is the
  /// return value; the statuses are then not written.
  auto decompress_batch(std::span<const std::span<const std::byte>> srcs, std::span<const std::span<std::byte>> dsts,
                        const batch_stream_index* ix, Container container, std::span<DecompressStatus> statuses) -> CompressStatus {
    if (!ctx_) return init_;
    const std::size_t k = srcs.size();
    if (dsts.size() != k || statuses.size() != k) return CompressStatus::InvalidArgument;
    if (ix != nullptr && (ix->items() != k || ix->first.size() != k + 1 || ix->offsets.size() != ix->first[k] ||
                          (!ix->regions.empty() && ix->regions.size() != (ix->first[k] - k) * SFH_SUBINDEX_WORDS)))
      return CompressStatus::InvalidArgument;
    std::vector<const void*> sp(k);
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> n(k), dn(k);
    std::vector<std::uint32_t> st(k);
    for (std::size_t i = 0; i < k; ++i) {
      sp[i] = srcs[i].data();
      n[i] = srcs[i].size();
      dp[i] = dsts[i].data();
      dn[i] = dsts[i].size();
    }
    const int rc = sfh_decompress_batch(ctx_, k, sp.data(), n.data(), ix ? ix->offsets.data() : nullptr,
                                        (ix && !ix->regions.empty()) ? ix->regions.data() : nullptr, dp.data(), dn.data(),
                                        ix ? ix->block_bytes.data() : nullptr, detail::to_c(container), st.data());
    if (rc != SFH_OK) return detail::to_status(rc);
    for (std::size_t i = 0; i < k; ++i) statuses[i] = st[i] > 7 ? DecompressStatus::Error : static_cast<DecompressStatus>(st[i]);
    return CompressStatus::Success;
  }
  /// index of the last compress call on this object (with_regions: also the per-region sub-index)
  auto index(bool with_regions = true) -> compat::expected<stream_index, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    stream_index ix;
    const std::size_t n = sfh_index_entries(ctx_);
    if (n == 0) return compat::unexpected{CompressStatus::InvalidArgument};
    ix.offsets.resize(n);
    ix.block_bytes = sfh_last_block_bytes(ctx_);
    ix.total_bytes = last_n_;
    int rc = sfh_copy_index(ctx_, ix.offsets.data(), n, 0, nullptr);
    if (rc == SFH_OK && with_regions) {
      ix.regions.resize((n - 1) * SFH_SUBINDEX_WORDS);
      rc = sfh_copy_subindex(ctx_, ix.regions.data(), ix.regions.size(), 0, nullptr);
    }
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    return ix;
  }
  /// decompress() on the GPU for an indexed stream: same statuses as the serial one (src/decompress.hpp:13-23),
  /// reported for the first failing segment in stream order.  dst.size() is the exact output size.
  /// A problem on the device side (no device, allocation) is DecompressStatus::Error.
  auto decompress(std::span<const std::byte> src, std::span<std::byte> dst, const stream_index& ix) -> DecompressStatus {
    if (!ctx_ || ix.offsets.size() < 2 || (!ix.regions.empty() && ix.regions.size() != ix.segments() * SFH_SUBINDEX_WORDS))
      return DecompressStatus::Error;
    std::uint32_t st = 0;
    const int rc = sfh_decompress(ctx_, src.data(), src.size(), ix.offsets.data(), ix.regions.empty() ? nullptr : ix.regions.data(),
                                  ix.segments(), dst.data(), dst.size(), ix.block_bytes, &st);
    if (rc != SFH_OK || st > 7) return DecompressStatus::Error;
    return static_cast<DecompressStatus>(st);
  }
  /// Random access: output bytes [offset, offset + dst.size()) of an indexed stream whose whole output is ix.total_bytes
  /// bytes (index() fills it in; an index from elsewhere sets it), for roughly what they hold: only the range's decode span -- from the
  /// start of the strip (ix.block_bytes) that holds its first byte to the segment that holds its last -- is uploaded and
  /// decoded (sfh_decompress_ranges).  The status is that of the span's first failing segment; dst is written only on
  /// Success.  A refused call (arguments) or a problem on the device side is DecompressStatus::Error, as in decompress().
  auto decompress_range(std::span<const std::byte> src, std::span<std::byte> dst, const stream_index& ix, std::uint64_t offset)
      -> DecompressStatus {
    const std::span<std::byte> d[1] = {dst};
    DecompressStatus st = DecompressStatus::Error;
    if (decompress_ranges(src, ix, std::span<const std::uint64_t>{&offset, 1}, d, std::span<DecompressStatus>{&st, 1}) !=
        CompressStatus::Success)
      return DecompressStatus::Error;
    return st;
  }
  /// Many ranges of one stream in one call: bytes [offsets[r], offsets[r] + dsts[r].size()) into dsts[r] (any addresses, not
  /// overlapping; ranges may overlap each other), range r's status into statuses[r]; one range's failure changes no other.
  /// A refused call (arguments, no device) is the return value, as with decompress_batch(); the statuses are then not written.
  auto decompress_ranges(std::span<const std::byte> src, const stream_index& ix, std::span<const std::uint64_t> offsets,
                         std::span<const std::span<std::byte>> dsts, std::span<DecompressStatus> statuses) -> CompressStatus {
    if (!ctx_) return init_;
    const std::size_t k = offsets.size();
    if (dsts.size() != k || statuses.size() != k || ix.offsets.size() < 2 ||
        (!ix.regions.empty() && ix.regions.size() != ix.segments() * SFH_SUBINDEX_WORDS))
      return CompressStatus::InvalidArgument;
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> len(k);
    std::vector<std::uint32_t> st(k);
    for (std::size_t i = 0; i < k; ++i) {
      dp[i] = dsts[i].data();
      len[i] = dsts[i].size();
    }
    const int rc = sfh_decompress_ranges(ctx_, src.data(), src.size(), ix.offsets.data(), ix.regions.empty() ? nullptr : ix.regions.data(),
                                         ix.segments(), ix.total_bytes, ix.block_bytes, k, offsets.data(), len.data(), dp.data(), st.data());
    if (rc != SFH_OK) return detail::to_status(rc);
    for (std::size_t i = 0; i < k; ++i) statuses[i] = st[i] > 7 ? DecompressStatus::Error : static_cast<DecompressStatus>(st[i]);
    return CompressStatus::Success;
  }
  /// A file written with Container::Dictzip (or any dictzip file of 32 KiB chunks) decoded with the index its own header
  /// carries (sfh_decompress_dz): the header, ISIZE and the CRC-32 are verified.  dst.size() >= ISIZE; *produced (nullable) =
  /// ISIZE on Success.  A file without such a table is decoded by decompress(src, dst, Container::Gzip), and so is whatever
  /// the GPU does not report Success for: the caller always gets the reference's answer.
  auto decompress_dz(std::span<const std::byte> src, std::span<std::byte> dst, std::size_t* produced = nullptr) -> DecompressStatus {
    if (ctx_) {
      std::uint32_t st = 0;
      std::uint64_t n = 0;
      const int rc = sfh_decompress_dz(ctx_, src.data(), src.size(), dst.data(), dst.size(), &n, &st);
      if (rc == SFH_OK && st == 0) {
        if (produced != nullptr) *produced = static_cast<std::size_t>(n);
        return DecompressStatus::Success;
      }
    }
    const auto st = decompress(src, dst, Container::Gzip);
    if (st == DecompressStatus::Success && produced != nullptr && src.size() >= 18) {
      const auto tr = src.last(4);
      *produced = detail::u8(tr[0]) | (detail::u8(tr[1]) << 8U) | (detail::u8(tr[2]) << 16U) | (detail::u8(tr[3]) << 24U);
    }
    return st;
  }
  /// Random access into such a file, given nothing but its bytes: output bytes [offset, offset + part.size()) into `part`
  /// (sfh_decompress_dz_ranges: the header is read on the host, only the chunks holding the range are uploaded and decoded;
  /// no checksum is verified).  A file without a table of 32 KiB chunks, a refused call or a device problem is Error.
  auto decompress_dz_range(std::span<const std::byte> src, std::span<std::byte> part, std::uint64_t offset) -> DecompressStatus {
    if (!ctx_) return DecompressStatus::Error;
    void* dp[1] = {part.data()};
    const std::uint64_t len = part.size();
    std::uint32_t st = 0;
    const int rc = sfh_decompress_dz_ranges(ctx_, src.data(), src.size(), 1, &offset, &len, dp, &st);
    if (rc != SFH_OK || st > 7) return DecompressStatus::Error;
    return static_cast<DecompressStatus>(st);
  }
  /// Random access into a BGZF file, given nothing but its bytes: output bytes [offset, offset + part.size()) into `part`
  /// (sfh_decompress_bgzf_ranges: the members are walked on the host, only the members holding the range are uploaded and
  /// decoded; each is checked for its wrapper, its ISIZE and the size of its body; no checksum is verified).  A refused call
  /// or a device problem is Error; `part` is written only on Success.
  auto decompress_bgzf_range(std::span<const std::byte> file, std::span<std::byte> part, std::uint64_t offset) -> DecompressStatus {
    if (!ctx_) return DecompressStatus::Error;
    void* dp[1] = {part.data()};
    const std::uint64_t len = part.size();
    std::uint32_t st = 0;
    const int rc = sfh_decompress_bgzf_ranges(ctx_, file.data(), file.size(), nullptr, nullptr, nullptr, 1, &offset, &len, dp, &st);
    if (rc != SFH_OK || st > 7) return DecompressStatus::Error;
    return static_cast<DecompressStatus>(st);
  }
  /// Many ranges of one BGZF file in one call: bytes [offsets[r], offsets[r] + parts[r].size()) into parts[r] (any addresses,
  /// not overlapping; ranges may overlap each other), range r's status into statuses[r]; one range's failure changes no other.
  /// ix (nullable): bgzf_read_index()'s, reusable across calls; without one the members are walked first.  A refused call
  /// (arguments, no device) is the return value; the statuses are then not written.
  auto decompress_bgzf_ranges(std::span<const std::byte> file, std::span<const std::uint64_t> offsets,
                              std::span<const std::span<std::byte>> parts, std::span<DecompressStatus> statuses,
                              const bgzf_index* ix = nullptr) -> CompressStatus {
    if (!ctx_) return init_;
    const std::size_t k = offsets.size();
    if (parts.size() != k || statuses.size() != k) return CompressStatus::InvalidArgument;
    if (ix != nullptr && (ix->member_off.empty() || ix->out_off.size() != ix->member_off.size())) return CompressStatus::InvalidArgument;
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> len(k);
    std::vector<std::uint32_t> st(k);
    for (std::size_t i = 0; i < k; ++i) {
      dp[i] = parts[i].data();
      len[i] = parts[i].size();
    }
    sfh_bgzf_info info{};
    if (ix != nullptr) info = sfh_bgzf_info{ix->total_bytes, static_cast<std::uint32_t>(ix->members()), ix->max_isize, ix->has_eof ? 1U : 0U, 0U};
    const int rc = sfh_decompress_bgzf_ranges(ctx_, file.data(), file.size(), ix ? ix->member_off.data() : nullptr,
                                              ix ? ix->out_off.data() : nullptr, ix ? &info : nullptr, k, offsets.data(), len.data(),
                                              dp.data(), st.data());
    if (rc != SFH_OK) return detail::to_status(rc);
    for (std::size_t i = 0; i < k; ++i) statuses[i] = st[i] > 7 ? DecompressStatus::Error : static_cast<DecompressStatus>(st[i]);
    return CompressStatus::Success;
  }
  /// The index of a stream given alone, recovered on the GPU from its flush markers: offsets of its
  /// max(1, ceil(dst_size / 32768)) segments + 1; block_bytes 0 (unknown), no regions.  A stream that is not block-flushed
  /// every 32 KiB is CompressStatus::NotIndexable.
  auto recover_index(std::span<const std::byte> src, std::size_t dst_size, Container container)
      -> compat::expected<stream_index, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    stream_index ix;
    const std::size_t nseg = dst_size ? (dst_size + SFH_SEGMENT_BYTES - 1) / SFH_SEGMENT_BYTES : 1;
    ix.offsets.resize(nseg + 1);
    ix.block_bytes = 0;
    ix.total_bytes = dst_size;
    const int rc = sfh_recover_index(ctx_, src.data(), src.size(), detail::to_c(container), dst_size,
                                     ix.offsets.data(), nseg, nullptr);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    return ix;
  }
  /// decompress(src, dst) for a stream given alone: on the GPU when its segment index can be recovered
  /// (sfh_decompress_any), else -- and whenever the GPU reports anything but Success -- container.hpp's serial
  /// decompress(src, dst, container), whose status is returned: the caller always gets the reference's answer.
  auto decompress(std::span<const std::byte> src, std::span<std::byte> dst, Container container) -> DecompressStatus {
    if (ctx_) {
      std::uint32_t st = 0;
      const int rc = sfh_decompress_any(ctx_, src.data(), src.size(), detail::to_c(container), dst.data(), dst.size(),
                                        dst.size(), nullptr, &st);
      if (rc == SFH_OK && st == 0) return DecompressStatus::Success;
    }
    return starflate::decompress(src, dst, container);
  }
  /// Many streams given alone, decoded in one call (sfh_decompress_any_batch): srcs[i] into exactly dsts[i].size() bytes at
  /// dsts[i] -- what compress_batch() wrote, read back with nothing but the streams.  As decompress(src, dst, container) does
  /// for one stream, every item the GPU did not report Success for (not block-flushed, damaged, a refused call) goes through
  /// container.hpp's serial decompress(srcs[i], dsts[i], container): statuses[i] is always the reference's answer.
  auto decompress_batch(std::span<const std::span<const std::byte>> srcs, std::span<const std::span<std::byte>> dsts,
                        Container container, std::span<DecompressStatus> statuses) -> CompressStatus {
    const std::size_t k = srcs.size();
    if (dsts.size() != k || statuses.size() != k) return CompressStatus::InvalidArgument;
    std::vector<std::uint32_t> st(k, 1U);
    if (ctx_ && k) {
      std::vector<const void*> sp(k);
      std::vector<void*> dp(k);
      std::vector<std::uint64_t> n(k), dn(k);
      for (std::size_t i = 0; i < k; ++i) {
        sp[i] = srcs[i].data();
        n[i] = srcs[i].size();
        dp[i] = dsts[i].data();
        dn[i] = dsts[i].size();
      }
      if (sfh_decompress_any_batch(ctx_, k, sp.data(), n.data(), detail::to_c(container), dp.data(), dn.data(), dn.data(),
                                   nullptr, st.data()) != SFH_OK)
        st.assign(k, 1U);
    }
    for (std::size_t i = 0; i < k; ++i)
      statuses[i] = st[i] == 0 ? DecompressStatus::Success : starflate::decompress(srcs[i], dsts[i], container);
    return CompressStatus::Success;
  }
  /// The indexes of many streams given alone, recovered on the GPU in one call (sfh_recover_index_batch): batch_index()'s
  /// layout with block_bytes 0 (unknown) and no regions.  indexable[i] (may be empty: not wanted) is false for an item that is
  /// not block-flushed every 32 KiB, whose entries are 0.
  auto recover_index_batch(std::span<const std::span<const std::byte>> srcs, std::span<const std::size_t> dst_sizes,
                           Container container, std::vector<bool>* indexable = nullptr)
      -> compat::expected<batch_stream_index, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    const std::size_t k = srcs.size();
    if (dst_sizes.size() != k) return compat::unexpected{CompressStatus::InvalidArgument};
    batch_stream_index ix;
    ix.block_bytes.assign(k, 0U);
    ix.first.resize(k + 1);
    std::vector<const void*> sp(k);
    std::vector<std::uint64_t> n(k), dn(k);
    std::vector<std::uint32_t> st(k);
    for (std::size_t i = 0; i < k; ++i) {
      sp[i] = srcs[i].data();
      n[i] = srcs[i].size();
      dn[i] = dst_sizes[i];
      ix.first[i + 1] = ix.first[i] + (dst_sizes[i] ? (dst_sizes[i] + SFH_SEGMENT_BYTES - 1) / SFH_SEGMENT_BYTES : 1) + 1;
    }
    ix.offsets.resize(ix.first[k]);
    const int rc = sfh_recover_index_batch(ctx_, k, sp.data(), n.data(), detail::to_c(container), dn.data(),
                                           ix.offsets.data(), st.data());
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    if (indexable != nullptr) {
      indexable->resize(k);
      for (std::size_t i = 0; i < k; ++i) (*indexable)[i] = st[i] == 0;
    }
    return ix;
  }
  /// decompress(src, dst, produced) for a raw, zlib or gzip stream (one member) with no index and no flush points, on the GPU
  /// from block discovery to the last byte (sfh_inflate_stream): the status and, on Success, the bytes are container.hpp's
  /// decompress(src, dst, container)'s, except that a zlib dst may be larger than the output (the Adler-32 covers the bytes
  /// produced; container.hpp checks it over all of dst); *produced (may be null) = the bytes the body produced.  A problem on the device side
  /// (no device, allocation) is DecompressStatus::Error; there is no host fallback.
  /// Container::GzipMembers (here and in decompress_stream_batch only): a file of gzip members, every member decoded behind
  /// the one before it -- decompress_members()'s statuses and bytes, with the one difference starflate_hip.h states (the
  /// trailers' values are checked after every body has decoded).
  auto decompress_stream(std::span<const std::byte> src, std::span<std::byte> dst, Container container, std::size_t* produced = nullptr)
      -> DecompressStatus {
    if (produced) *produced = 0;
    if (!ctx_) return DecompressStatus::Error;
    std::uint32_t st = 0;
    std::uint64_t n = 0;
    // (an empty dst still decodes: the size query is the C interface's, with a null dst)
    std::byte dummy{};
    void* d = dst.empty() ? static_cast<void*>(&dummy) : static_cast<void*>(dst.data());
    const int rc = sfh_inflate_stream(ctx_, src.data(), src.size(), detail::to_c(container), d, dst.size(), &n, &st);
    if (rc != SFH_OK || st > 7) return DecompressStatus::Error;
    if (produced) *produced = static_cast<std::size_t>(n);
    return static_cast<DecompressStatus>(st);
  }
  /// decompress_stream() on many streams in one call (sfh_inflate_stream_batch): srcs[i] into dsts[i], its status into
  /// statuses[i] and, when `produced` is not empty, the bytes its body produced into produced[i] -- for every item exactly what
  /// decompress_stream(srcs[i], dsts[i], container) gives on it alone.  dsts[i] is written only where statuses[i] is Success
  /// (or the checksum did not match).  A refused call (arguments) is the return value, the statuses then not written; a
  /// problem on the device side (no device, allocation) is returned as well and makes every status Error.  No host fallback.
  auto decompress_stream_batch(std::span<const std::span<const std::byte>> srcs, std::span<const std::span<std::byte>> dsts,
                               Container container, std::span<DecompressStatus> statuses, std::span<std::size_t> produced = {})
      -> CompressStatus {
    const std::size_t k = srcs.size();
    if (dsts.size() != k || statuses.size() != k || (!produced.empty() && produced.size() != k)) return CompressStatus::InvalidArgument;
    if (!ctx_) {
      for (auto& st : statuses) st = DecompressStatus::Error;
      return init_;
    }
    std::vector<const void*> sp(k);
    std::vector<void*> dp(k);
    std::vector<std::uint64_t> n(k), cap(k), out(k);
    std::vector<std::uint32_t> st(k);
    static std::byte dummy{};  // (an empty dst still decodes: a null one is the C interface's size query)
    for (std::size_t i = 0; i < k; ++i) {
      sp[i] = srcs[i].data();
      n[i] = srcs[i].size();
      dp[i] = dsts[i].empty() ? static_cast<void*>(&dummy) : static_cast<void*>(dsts[i].data());
      cap[i] = dsts[i].size();
    }
    const int rc = sfh_inflate_stream_batch(ctx_, k, sp.data(), n.data(), detail::to_c(container), dp.data(), cap.data(),
                                            out.data(), st.data());
    if (rc == SFH_E_INVALID_ARG) return CompressStatus::InvalidArgument;
    for (std::size_t i = 0; i < k; ++i) {
      statuses[i] = (rc != SFH_OK || st[i] > 7) ? DecompressStatus::Error : static_cast<DecompressStatus>(st[i]);
      if (!produced.empty()) produced[i] = rc == SFH_OK ? static_cast<std::size_t>(out[i]) : 0;
    }
    return rc == SFH_OK ? CompressStatus::Success : detail::to_status(rc);
  }
  /// device pointers (src 16-byte aligned), optional hipStream_t
  auto compress_device(const void* d_src, std::size_t n, void* d_dst, std::size_t cap, const compress_options& opt = {},
                       void* stream = nullptr) -> compat::expected<std::size_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    const auto c = detail::to_c(opt);
    std::size_t out = 0;
    const int rc = sfh_compress_device(ctx_, d_src, n, d_dst, cap, &out, &c, stream);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    last_n_ = n;
    return out;
  }
  /// enqueue only: the stream size is left in *d_out_n, a device word (what gather_streams reads)
  auto compress_device_async(const void* d_src, std::size_t n, void* d_dst, std::size_t cap, std::uint64_t* d_out_n,
                             const compress_options& opt = {}, void* stream = nullptr) -> CompressStatus {
    if (!ctx_) return init_;
    const auto c = detail::to_c(opt);
    const int rc = sfh_compress_device_async(ctx_, d_src, n, d_dst, cap, d_out_n, &c, stream);
    if (rc == SFH_OK) last_n_ = n;
    return detail::to_status(rc);
  }

  /// One process per GPU: what every rank of an RCCL communicator calls after compressing its shard (whole strips,
  /// final_stream = false on every rank but the last).  The byte-aligned streams are put back to back, in rank order, at
  /// d_out + base on `root`: one ncclAllGather of the sizes, then one point-to-point transfer per peer (no ring, no
  /// all-reduce) -- legal because a match only has to stay inside the bytes already written
  /// (/root/reference/src/decompress.cpp:178) and blocks simply follow one another until BFINAL (:410-415).
  /// nccl_comm: an ncclComm_t.  base / cap: the root's (bytes already in d_out, its capacity), the same on every rank.
  /// Returns the end of the concatenation; `sizes` (optional) receives every rank's stream size.
  auto gather_streams(void* nccl_comm, int root, const void* d_stream, const std::uint64_t* d_size, void* d_out, std::uint64_t base,
                      std::uint64_t cap, void* stream = nullptr, std::vector<std::uint64_t>* sizes = nullptr)
      -> compat::expected<std::uint64_t, CompressStatus> {
    if (!ctx_) return compat::unexpected{init_};
    int nranks = 0, rank = 0;
    if (const int rc = sfh_comm_ranks(nccl_comm, &nranks, &rank); rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    std::vector<std::uint64_t> local(static_cast<std::size_t>(nranks));
    std::uint64_t end = 0;
    const int rc = sfh_gather_streams(ctx_, nccl_comm, root, d_stream, d_size, d_out, base, cap, local.data(), &end, stream);
    if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
    if (sizes != nullptr) *sizes = std::move(local);
    return end;
  }
};

/// One process, several GPUs: contiguous shards of `src` on the given compressors (one per device), one stream
/// in `dst`, bit-identical to a single compress() call.
inline auto compress(std::span<compressor* const> gpus, std::span<const std::byte> src, std::span<std::byte> dst,
                     const compress_options& opt = {}) -> compat::expected<std::size_t, CompressStatus> {
  std::vector<sfh_ctx*> h;
  for (const auto* g : gpus) {
    if (g == nullptr || g->native() == nullptr) return compat::unexpected{g != nullptr ? g->status() : CompressStatus::InvalidArgument};
    h.push_back(g->native());
  }
  const auto c = detail::to_c(opt);
  std::size_t n = 0;
  const int rc = sfh_compress_multi(h.data(), static_cast<int>(h.size()), src.data(), src.size(), dst.data(), dst.size(), &n, &c);
  if (rc != SFH_OK) return compat::unexpected{detail::to_status(rc)};
  return n;
}

namespace detail {
inline auto thread_compressors() -> std::vector<std::pair<int, compressor>>& {
  thread_local std::vector<std::pair<int, compressor>> cache;
  return cache;
}
/// The calling thread's context for `device`, created on first use and kept until the thread exits or calls
/// release_thread_compressor(): the free function below does not pay for a stream, events and device scratch on
/// every call.  A context holds device scratch sized by its largest call (2.3 bytes per input byte, at most 2.3 GiB).
inline auto thread_compressor(int device) -> compressor& {
  auto& cache = thread_compressors();
  for (auto& e : cache)
    if (e.first == device) return e.second;
  cache.emplace_back(device, compressor{device});
  return cache.back().second;
}
}  // namespace detail

/// Frees the calling thread's cached context(s) -- stream, events, device scratch -- for `device`, or for every
/// device with -1.  The next free-function compress() on this thread makes a new one.  Returns how many were freed.
inline auto release_thread_compressor(int device = -1) -> std::size_t {
  auto& cache = detail::thread_compressors();
  const auto before = cache.size();
  std::erase_if(cache, [device](const auto& e) { return device < 0 || e.first == device; });
  return before - cache.size();
}

/// Compresses `src` into `dst` (dst.size() >= compress_bound(src.size())); returns the stream size.
/// Re-entrant like the reference's decompress() (src/decompress.hpp:63-71): each thread keeps its own context per device.
inline auto compress(std::span<const std::byte> src, std::span<std::byte> dst, const compress_options& opt = {})
    -> compat::expected<std::size_t, CompressStatus> {
  return detail::thread_compressor(opt.device).compress(src, dst, opt);
}

}  // namespace starflate
