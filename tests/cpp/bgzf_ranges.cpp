// GPU test of the C++23 BGZF random access: compressor::decompress_bgzf_range / decompress_bgzf_ranges on a file from
// compressor::compress_bgzf and on a file of bgzip's 65280-byte members (argv[2], its payload argv[3]: written by
// tests/test_gpu_bgzf_ranges_cpp.py with Python's zlib), and starflate::bgzf_voffsets_to_offsets / bgzf_offsets_to_voffsets.
// argv[1] = tests/golden.
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
  if (argc < 4) return 2;
  const auto html = read_file(std::string{argv[1]} + "/starfleet.html");
  compressor gpu{0};
  if (gpu.status() != CompressStatus::Success) {
    std::printf("no device: status %d\n", static_cast<int>(gpu.status()));
    return 2;
  }
  int fail = 0;
  const auto check = [&](bool ok, const char* what) {
    if (!ok) {
      std::printf("failed: %s\n", what);
      ++fail;
    }
  };
  Bytes in;  // 5 members and a few bytes
  while (in.size() < 5 * 32768 + 77) in.insert(in.end(), html.begin(), html.end());
  in.resize(5 * 32768 + 77);
  Bytes own(bgzf_bound(in.size()));
  const auto sz = gpu.compress_bgzf(in, own);
  check(sz.has_value(), "compress_bgzf");
  if (!sz.has_value()) return 1;
  own.resize(*sz);
  const Bytes wide = read_file(argv[2]), wide_in = read_file(argv[3]);

  const auto run = [&](const Bytes& file, const Bytes& data, const char* what) {
    const auto ix = bgzf_read_index(file);
    check(ix.has_value() && ix->total_bytes == data.size(), what);
    if (!ix.has_value()) return;
    // one range: inside a member, across a member boundary, the last bytes, nothing
    const std::uint64_t b1 = ix->out_off[1];
    const std::uint64_t offs[4] = {100, b1 - 3, data.size() - 5, data.size()};
    const std::size_t lens[4] = {4096, 6, 5, 0};
    for (int k = 0; k < 4; ++k) {
      Bytes part(lens[k] + 2, std::byte{0xA5});
      const auto st = gpu.decompress_bgzf_range(file, std::span{part}.subspan(1, lens[k]), offs[k]);
      check(st == DecompressStatus::Success && std::memcmp(part.data() + 1, data.data() + offs[k], lens[k]) == 0 &&
                part.front() == std::byte{0xA5} && part.back() == std::byte{0xA5},
            what);
    }
    Bytes one(1);
    check(gpu.decompress_bgzf_range(file, one, data.size()) == DecompressStatus::Error, "a range behind the file: refused");
    // many ranges into one packed buffer, with and without the index
    const std::vector<std::uint64_t> many = {0, b1 - 1, ix->out_off[2] - 40000, 7, data.size() - 1};
    const std::vector<std::size_t> mlen = {1, 2, 50000, 3, 1};
    for (const bgzf_index* given : {static_cast<const bgzf_index*>(nullptr), &*ix}) {
      Bytes pack(50007, std::byte{0});
      std::vector<std::span<std::byte>> parts;
      std::size_t at = 0;
      for (const std::size_t n : mlen) {
        parts.push_back(std::span{pack}.subspan(at, n));
        at += n;
      }
      std::vector<DecompressStatus> st(many.size(), DecompressStatus::Error);
      check(gpu.decompress_bgzf_ranges(file, many, parts, st, given) == CompressStatus::Success, what);
      for (std::size_t r = 0; r < many.size(); ++r)
        check(st[r] == DecompressStatus::Success && std::memcmp(parts[r].data(), data.data() + many[r], mlen[r]) == 0, what);
    }
    // virtual offsets from the index fetch the bytes of the offsets they translate to
    const std::vector<std::uint64_t> vs = {ix->member_off[1] << 16U | 5U, ix->member_off[0] << 16U, ix->member_off[1] << 16U | 0xFFFFU,
                                           ix->member_off.back() << 16U};
    const auto os = bgzf_voffsets_to_offsets(*ix, vs);
    check(os.size() == 4 && os[0] == b1 + 5 && os[1] == 0 && os[3] == data.size(), "voffsets -> offsets");
    check(os[2] == (ix->out_off[2] - b1 >= 0xFFFFU ? b1 + 0xFFFFU : ~std::uint64_t{0}), "uoffset behind the member");
    const auto back = bgzf_offsets_to_voffsets(*ix, std::span{os}.first(2));
    check(back.size() == 2 && back[0] == vs[0] && back[1] == vs[1], "offsets -> voffsets");
    Bytes part(100);
    check(gpu.decompress_bgzf_range(file, part, os[0]) == DecompressStatus::Success &&
              std::memcmp(part.data(), data.data() + b1 + 5, 100) == 0,
          "a virtual offset's bytes");
  };
  run(own, in, "a file from compress_bgzf");
  run(wide, wide_in, "65280-byte members");
  // a damaged member: its ranges fail, `part` is left alone, the others are exact
  {
    const auto ix = bgzf_read_index(wide);
    if (ix.has_value()) {
      Bytes bad = wide;
      bad[static_cast<std::size_t>(ix->member_off[1]) + 2] = std::byte{7};  // CM
      Bytes a(10, std::byte{0xA5}), b(10, std::byte{0xA5});
      const std::vector<std::uint64_t> offs = {ix->out_off[1] + 9, 9};
      const std::vector<std::span<std::byte>> parts = {a, b};
      std::vector<DecompressStatus> st(2, DecompressStatus::Success);
      check(gpu.decompress_bgzf_ranges(bad, offs, parts, st, &*ix) == CompressStatus::Success, "a damaged member: the call");
      check(st[0] == DecompressStatus::Error && a == Bytes(10, std::byte{0xA5}), "a damaged member: its range");
      check(st[1] == DecompressStatus::Success && std::memcmp(b.data(), wide_in.data() + 9, 10) == 0, "a damaged member: the other range");
    }
  }
  std::printf(fail ? "%d checks failed\n" : "bgzf ranges ok (%d failures)\n", fail);
  return fail ? 1 : 0;
}
