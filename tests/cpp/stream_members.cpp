// GPU test of Container::GzipMembers through the C++23 interface: three buffers compressed as gzip streams, joined with zero
// bytes between them, and read back by compressor::decompress_stream and decompress_stream_batch.  Statuses and bytes are
// compared with the host specification, starflate::decompress(src, dst, Container::GzipMembers) (container.hpp), on the intact
// file, on one with a flipped CRC bit and on one cut inside its last trailer.
#include "starflate/compress.hpp"
#include "starflate/container.hpp"

#include <cstdio>
#include <span>
#include <vector>

using Bytes = std::vector<std::byte>;

static auto text(std::size_t n, unsigned seed) -> Bytes {
  static const char* words[] = {"alpha ", "beta ", "gamma ", "delta ", "members ", "of ", "a ", "gzip ", "file\n"};
  Bytes b;
  unsigned x = seed * 2654435761U + 1U;
  while (b.size() < n) {
    x = x * 1664525U + 1013904223U;
    for (const char* w = words[(x >> 16U) % 9U]; *w != 0 && b.size() < n; ++w) b.push_back(static_cast<std::byte>(*w));
  }
  return b;
}

int main() {
  using namespace starflate;
  compressor gpu{0};
  if (gpu.status() != CompressStatus::Success) {
    std::printf("no context\n");
    return 1;
  }
  Bytes file, want;
  compress_options opt;
  opt.container = Container::Gzip;
  for (const std::size_t n : {std::size_t{70000}, std::size_t{0}, std::size_t{1234}}) {
    const Bytes part = text(n, static_cast<unsigned>(n));
    Bytes z(compress_bound(part.size()) + 64);  // (the wrapper: 18 bytes)
    const auto r = gpu.compress(part, z, opt);
    if (!r) {
      std::printf("compress failed\n");
      return 1;
    }
    file.insert(file.end(), z.begin(), z.begin() + static_cast<std::ptrdiff_t>(*r));
    file.insert(file.end(), 5, std::byte{0});
    want.insert(want.end(), part.begin(), part.end());
  }
  Bytes bad_crc = file, cut = file;
  bad_crc[40] ^= std::byte{0x10};  // (inside the first body or not: the host says which status)
  cut.resize(cut.size() - 5 - 3);
  int fail = 0;
  std::vector<Bytes> files{file, bad_crc, cut};
  std::vector<Bytes> outs(3, Bytes(want.size() + 100)), host(3, Bytes(want.size() + 100));
  std::vector<DecompressStatus> single(3);
  for (std::size_t i = 0; i < 3; ++i) {
    std::size_t n = 0;
    single[i] = gpu.decompress_stream(files[i], outs[i], Container::GzipMembers, &n);
    const auto hs = decompress(std::span<const std::byte>(files[i]), std::span<std::byte>(host[i]), Container::GzipMembers);
    if (single[i] != hs) {
      std::printf("file %zu: GPU status %d, host %d\n", i, static_cast<int>(single[i]), static_cast<int>(hs));
      ++fail;
    }
    if (hs == DecompressStatus::Success && (n != want.size() || !std::equal(want.begin(), want.end(), outs[i].begin()))) {
      std::printf("file %zu: not the input back\n", i);
      ++fail;
    }
  }
  if (single[0] != DecompressStatus::Success || single[2] != DecompressStatus::SrcTooSmall) {
    std::printf("statuses %d, %d, %d\n", static_cast<int>(single[0]), static_cast<int>(single[1]), static_cast<int>(single[2]));
    ++fail;
  }
  std::vector<Bytes> bouts(3, Bytes(want.size() + 100));
  std::vector<std::span<const std::byte>> srcs(files.begin(), files.end());
  std::vector<std::span<std::byte>> dsts(bouts.begin(), bouts.end());
  std::vector<DecompressStatus> st(3);
  std::vector<std::size_t> produced(3);
  if (gpu.decompress_stream_batch(srcs, dsts, Container::GzipMembers, st, produced) != CompressStatus::Success) {
    std::printf("decompress_stream_batch refused\n");
    ++fail;
  }
  for (std::size_t i = 0; i < 3; ++i)
    if (st[i] != single[i] || (st[i] == DecompressStatus::Success && (produced[i] != want.size() || bouts[i] != outs[i]))) {
      std::printf("batch item %zu differs from the single call\n", i);
      ++fail;
    }
  // every other decoder keeps refusing the container
  std::vector<std::byte> d(want.size());
  std::uint32_t any_st = 0;
  if (sfh_decompress_any(gpu.native(), file.data(), file.size(), SFH_GZIP_MEMBERS, d.data(), d.size(), d.size(), nullptr, &any_st) !=
      SFH_E_INVALID_ARG) {
    std::printf("sfh_decompress_any took SFH_GZIP_MEMBERS\n");
    ++fail;
  }
  if (fail == 0) std::printf("ok\n");
  return fail != 0;
}
