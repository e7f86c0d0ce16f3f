// GPU test of the C++23 random-access members: compressor::decompress_range() and compressor::decompress_ranges() on a
// stream of this library with its index() -- with and without the sub-index -- must give the input's slices, at destinations
// packed back to back in one buffer whose other bytes stay untouched; a damaged segment fails only the ranges whose decode
// span holds it.  argv[1] = tests/golden.
#include "starflate/compress.hpp"

#include <cstdio>
#include <cstring>
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

auto main(int argc, char** argv) -> int {
  using namespace starflate;
  const std::string golden = argc > 1 ? argv[1] : "tests/golden";
  const auto html = read_file(golden + "/starfleet.html");
  compressor gpu{0};
  if (gpu.status() != CompressStatus::Success) {
    std::printf("no device: status %d\n", static_cast<int>(gpu.status()));
    return 2;
  }
  Bytes in;  // 600 KiB and a few bytes: the page over and over with noise in between
  std::uint32_t x = 2463534242U;
  while (in.size() < 600 * 1024 + 77) {
    in.insert(in.end(), html.begin(), html.end());
    for (int i = 0; i < 1500; ++i) in.push_back(static_cast<std::byte>((x = x * 1103515245U + 12345U) >> 24));
  }
  const std::uint64_t n = in.size();
  int fail = 0;
  for (const std::uint32_t bb : {32768U, 131072U}) {
    compress_options opt;
    opt.block_bytes = bb;
    Bytes stream(compress_bound(in.size()));
    const auto sz = gpu.compress(in, stream, opt);
    if (!sz) {
      std::printf("compress failed\n");
      return 1;
    }
    stream.resize(*sz);
    const auto ix = gpu.index();
    const auto ix_plain = gpu.index(false);
    if (!ix || !ix_plain || ix->block_bytes != bb || ix->total_bytes != n) {
      std::printf("index failed\n");
      return 1;
    }
    // ranges: edges of segments and strips, odd offsets and lengths, nothing at all, everything
    std::vector<std::uint64_t> offs{0, 1, 32767, 32768, bb - 1ULL, bb, bb + 1ULL, 3ULL * bb - 7, n - 1, n - 40000, 12345, n, 0};
    std::vector<std::uint64_t> lens{1, 32768, 2, 4097, 2, 1, 2ULL * bb, 70001, 1, 40000, 0, 0, n};
    for (int i = 0; i < 60; ++i) {
      const std::uint64_t o = (x = x * 1103515245U + 12345U) % n;
      const std::uint64_t l = (x = x * 1103515245U + 12345U) % 100000 % (n - o + 1);
      offs.push_back(o);
      lens.push_back(l);
    }
    const std::size_t k = offs.size();
    for (const auto* index : {&*ix, &*ix_plain}) {
      std::size_t total = 16;
      for (const auto l : lens) total += l;
      Bytes buf(total + 16, std::byte{0xA5}), want = buf;
      std::vector<std::span<std::byte>> dsts;
      std::size_t at = 5;
      for (std::size_t i = 0; i < k; ++i) {
        dsts.emplace_back(buf.data() + at, lens[i]);
        if (lens[i]) std::memcpy(want.data() + at, in.data() + offs[i], lens[i]);
        at += lens[i];
      }
      std::vector<DecompressStatus> st(k, DecompressStatus::Error);
      const auto rc = gpu.decompress_ranges(stream, *index, offs, dsts, st);
      if (rc != CompressStatus::Success) {
        std::printf("decompress_ranges refused: %d\n", static_cast<int>(rc));
        return 1;
      }
      for (std::size_t i = 0; i < k; ++i)
        if (st[i] != DecompressStatus::Success) {
          std::printf("block_bytes %u, range %zu: status %d\n", bb, i, static_cast<int>(st[i]));
          ++fail;
        }
      if (buf != want) {
        std::printf("block_bytes %u: bytes differ\n", bb);
        ++fail;
      }
      for (std::size_t i = 0; i < k; i += 7) {
        Bytes one(lens[i] + 2, std::byte{0x5A});
        const auto s1 = gpu.decompress_range(stream, std::span<std::byte>(one.data() + 1, lens[i]), *index, offs[i]);
        if (s1 != DecompressStatus::Success || (lens[i] && std::memcmp(one.data() + 1, in.data() + offs[i], lens[i]) != 0) ||
            one.front() != std::byte{0x5A} || one.back() != std::byte{0x5A}) {
          std::printf("block_bytes %u, decompress_range %zu: status %d or wrong bytes\n", bb, i, static_cast<int>(s1));
          ++fail;
        }
      }
    }
    // BTYPE 3 in segment 5's block header: only the ranges whose decode span holds it fail, and they are not written
    Bytes bad = stream;
    bad[static_cast<std::size_t>(ix->offsets[5])] |= std::byte{0x06};
    const std::uint64_t sps = bb / 32768;
    std::vector<Bytes> outs(k);
    std::vector<std::span<std::byte>> dsts;
    for (std::size_t i = 0; i < k; ++i) {
      outs[i].assign(lens[i], std::byte{0xA5});
      dsts.emplace_back(outs[i]);
    }
    std::vector<DecompressStatus> st(k, DecompressStatus::Success);
    if (gpu.decompress_ranges(bad, *ix, offs, dsts, st) != CompressStatus::Success) {
      std::printf("decompress_ranges refused the damaged stream\n");
      return 1;
    }
    for (std::size_t i = 0; i < k; ++i) {
      const bool holds = lens[i] != 0 && offs[i] / 32768 / sps * sps <= 5 && 5 <= (offs[i] + lens[i] - 1) / 32768;
      const bool sound = lens[i] == 0 || std::memcmp(outs[i].data(), in.data() + offs[i], lens[i]) == 0;
      const bool untouched = outs[i] == Bytes(lens[i], std::byte{0xA5});
      if (holds ? (st[i] != DecompressStatus::InvalidBlockHeader || !untouched) : (st[i] != DecompressStatus::Success || !sound)) {
        std::printf("block_bytes %u, damaged, range %zu (holds %d): status %d\n", bb, i, holds ? 1 : 0, static_cast<int>(st[i]));
        ++fail;
      }
    }
    // refused calls: a status span too short, a range behind the end
    {
      std::vector<DecompressStatus> few(k - 1);
      if (gpu.decompress_ranges(stream, *ix, offs, dsts, few) != CompressStatus::InvalidArgument) ++fail;
      Bytes o(10);
      if (gpu.decompress_range(stream, o, *ix, n - 5) != DecompressStatus::Error) ++fail;
    }
  }
  std::printf("decompress_ranges: %d failed\n", fail);
  return fail ? 1 : 0;
}
