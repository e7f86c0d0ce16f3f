// GPU test of the C++23 batch API: compressor::compress_batch() over items of mixed sizes, each stream decoded with
// starflate::decompress() (raw, zlib, gzip) and compared with the input and with the single call's stream.
// argv[1] = tests/golden.
#include "starflate/compress.hpp"
#include "starflate/decompress.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <span>
#include <string>
#include <vector>

static auto read_file(const std::string& path) -> std::vector<std::byte> {
  std::ifstream f{path, std::ios::binary};
  std::vector<char> c((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<std::byte> b(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) b[i] = static_cast<std::byte>(c[i]);
  return b;
}

auto main(int argc, char** argv) -> int {
  using namespace starflate;
  const std::string golden = argc > 1 ? argv[1] : "tests/golden";
  const auto html = read_file(golden + "/starfleet.html");
  compressor gpu{0};
  if (gpu.status() != CompressStatus::Success) {
    std::printf("no device: status %d\n", static_cast<int>(gpu.status()));
    return 2;
  }
  std::vector<std::vector<std::byte>> items{{}, {std::byte{'x'}}, html, std::vector<std::byte>(100000, std::byte{0})};
  std::vector<std::byte> big;  // 300 KiB of the page over and over, then a few bytes of noise
  while (big.size() < 300 * 1024) big.insert(big.end(), html.begin(), html.end());
  std::uint32_t x = 12345;
  for (int i = 0; i < 777; ++i) big.push_back(static_cast<std::byte>((x = x * 1103515245U + 12345U) >> 24));
  items.push_back(big);
  int fail = 0;
  for (const auto kind : {Container::Raw, Container::Zlib, Container::Gzip}) {
    compress_options opt;
    opt.container = kind;
    std::vector<std::vector<std::byte>> out;
    std::vector<std::span<const std::byte>> srcs;
    std::vector<std::span<std::byte>> dsts;
    for (const auto& in : items) out.emplace_back(compress_bound(in.size()));
    for (std::size_t i = 0; i < items.size(); ++i) {
      srcs.emplace_back(items[i]);
      dsts.emplace_back(out[i]);
    }
    std::vector<std::size_t> sizes(items.size());
    const auto r = gpu.compress_batch(srcs, dsts, sizes, opt);
    if (!r) {
      std::printf("compress_batch failed: %d\n", static_cast<int>(r.error()));
      ++fail;
      continue;
    }
    std::size_t total = 0;
    for (std::size_t i = 0; i < items.size(); ++i) {
      total += sizes[i];
      std::vector<std::byte> one(compress_bound(items[i].size()));
      const auto n = gpu.compress(items[i], one, opt);
      if (!n || *n != sizes[i] || !std::equal(one.begin(), one.begin() + static_cast<std::ptrdiff_t>(*n), out[i].begin())) {
        std::printf("item %zu (container %d): batch stream differs from the single call's\n", i, static_cast<int>(kind));
        ++fail;
      }
      std::vector<std::byte> back(items[i].size());
      const auto st = decompress(std::span<const std::byte>(out[i].data(), sizes[i]), back, kind);
      if (st != DecompressStatus::Success || back != items[i]) {
        std::printf("item %zu (container %d): round trip failed, status %d\n", i, static_cast<int>(kind), static_cast<int>(st));
        ++fail;
      }
    }
    if (total != *r) {
      std::printf("total %zu != %zu\n", *r, total);
      ++fail;
    }
  }
  // a destination below the bound is refused as a whole
  {
    std::vector<std::byte> small(8), ok(compress_bound(html.size()));
    const std::vector<std::span<const std::byte>> srcs{html, html};
    const std::vector<std::span<std::byte>> dsts{ok, small};
    std::vector<std::size_t> sizes(2);
    const auto r = gpu.compress_batch(srcs, dsts, sizes);
    if (r || r.error() != CompressStatus::DstTooSmall) {
      std::printf("a too-small destination was not refused\n");
      ++fail;
    }
  }
  std::printf("compress_batch: %d failed\n", fail);
  return fail ? 1 : 0;
}
