// GPU test of the C++23 batched stream decoder: compressor::decompress_stream_batch() over raw, zlib and gzip items of mixed
// sizes, intact and damaged, together with the golden DEFLATE fixtures.  Every item's status is compared with the host
// decoder's, starflate::decompress(src, dst, Container) (container.hpp), and every intact item's bytes with the input.
// argv[1] = tests/golden.
#include "starflate/compress.hpp"
#include "starflate/container.hpp"
#include "starflate/decompress.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <span>
#include <string>
#include <vector>

using Bytes = std::vector<std::byte>;

static auto read_file(const std::string& path) -> Bytes {
  std::ifstream f{path, std::ios::binary};
  std::vector<char> c((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  Bytes b(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) b[i] = static_cast<std::byte>(c[i]);
  return b;
}

// one batch call on `streams` (capacities `sizes`), every item against the host decoder on it alone
static auto check(starflate::compressor& gpu, const std::vector<Bytes>& streams, const std::vector<std::size_t>& sizes,
                  starflate::Container kind, const std::vector<const Bytes*>& want, const char* what) -> int {
  using namespace starflate;
  const std::size_t k = streams.size();
  std::vector<Bytes> out(k), host(k);
  std::vector<std::span<const std::byte>> srcs;
  std::vector<std::span<std::byte>> dsts;
  for (std::size_t i = 0; i < k; ++i) {
    out[i].assign(sizes[i], std::byte{0});
    host[i].assign(sizes[i], std::byte{0});
    srcs.emplace_back(streams[i]);
    dsts.emplace_back(out[i]);
  }
  std::vector<DecompressStatus> st(k);
  std::vector<std::size_t> produced(k);
  const auto rc = gpu.decompress_stream_batch(srcs, dsts, kind, st, produced);
  if (rc != CompressStatus::Success) {
    std::printf("%s: decompress_stream_batch refused: %d\n", what, static_cast<int>(rc));
    return 1;
  }
  int fail = 0;
  for (std::size_t i = 0; i < k; ++i) {
    const auto hs = decompress(std::span<const std::byte>(streams[i]), std::span<std::byte>(host[i]), kind);
    if (st[i] != hs) {
      std::printf("%s, item %zu (container %d): GPU status %d, host %d\n", what, i, static_cast<int>(kind), static_cast<int>(st[i]),
                  static_cast<int>(hs));
      ++fail;
    }
    if (want[i] != nullptr && (st[i] != DecompressStatus::Success || produced[i] != want[i]->size() || out[i] != *want[i])) {
      std::printf("%s, item %zu (container %d): not the input back\n", what, i, static_cast<int>(kind));
      ++fail;
    }
    if (st[i] == DecompressStatus::Success && out[i] != host[i]) {
      std::printf("%s, item %zu (container %d): bytes differ from the host decoder's\n", what, i, static_cast<int>(kind));
      ++fail;
    }
  }
  return fail;
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
  std::vector<Bytes> items{{}, {std::byte{'x'}}, Bytes(html.begin(), html.begin() + 20000), html, Bytes(100000, std::byte{0})};
  Bytes big;
  while (big.size() < 300 * 1024) big.insert(big.end(), html.begin(), html.end());
  std::uint32_t x = 12345;
  for (int i = 0; i < 777; ++i) big.push_back(static_cast<std::byte>((x = x * 1103515245U + 12345U) >> 24));
  items.push_back(big);
  int fail = 0;
  for (const auto kind : {Container::Raw, Container::Zlib, Container::Gzip}) {
    compress_options opt;
    opt.container = kind;
    std::vector<Bytes> streams;
    std::vector<std::size_t> sizes;
    std::vector<const Bytes*> want;
    for (const auto& in : items) {
      Bytes out(compress_bound(in.size()));
      const auto n = gpu.compress(in, out, opt);
      if (!n) {
        std::printf("compress failed\n");
        return 1;
      }
      out.resize(*n);
      streams.push_back(out);
      sizes.push_back(in.size());
      want.push_back(&in);
    }
    const std::size_t intact = streams.size();
    // damaged copies between the intact items: truncated, BTYPE 3, a checksum byte, a capacity one short
    const std::size_t hdr = kind == Container::Raw ? 0 : kind == Container::Zlib ? 2 : 10;
    for (std::size_t i = 2; i < intact; ++i) {
      Bytes t = streams[i];
      t.resize(t.size() / 2);
      streams.push_back(t);
      Bytes b = streams[i];
      b[hdr] |= std::byte{0x06};
      streams.push_back(b);
      Bytes c = streams[i];
      c[c.size() - 1] ^= std::byte{0x20};
      streams.push_back(c);
      streams.push_back(streams[i]);
      for (int r = 0; r < 3; ++r) sizes.push_back(sizes[i]);
      sizes.push_back(sizes[i] - 1);
      for (int r = 0; r < 4; ++r) want.push_back(nullptr);
    }
    fail += check(gpu, streams, sizes, kind, want, "library streams");
  }
  const Bytes dyn = read_file(golden + "/starfleet.html.dynamic"), fix = read_file(golden + "/starfleet.html.fixed");
  fail += check(gpu, {dyn, fix, dyn}, {html.size(), html.size(), html.size()}, Container::Raw, {&html, &html, &html}, "golden");
  if (fail) return 1;
  std::printf("ok\n");
  return 0;
}
