// GPU test of the C++23 ZIP members: compressor::compress_zip writes an archive starflate::zip_read_index() walks and
// compressor::decompress_zip() reads back, entry by entry, in any order; an archive another tool wrote (argv[2], made by the
// test with zipfile: deflated and stored entries) decodes to the files beside it (argv[2] + ".<i>"); a damaged entry ends in
// a status.  argv[1] = tests/golden.
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
  int fail = 0;
  const auto check = [&](bool ok, const char* what) {
    if (!ok) {
      std::printf("failed: %s\n", what);
      ++fail;
    }
  };
  Bytes big;  // three segments and a few bytes
  while (big.size() < 3 * 32768 + 5) big.insert(big.end(), html.begin(), html.end());
  big.resize(3 * 32768 + 5);
  const Bytes none;
  const std::vector<std::string_view> names{"a", "dir/starfleet.html", "empty"};
  const std::vector<std::span<const std::byte>> srcs{big, html, none};
  const std::vector<std::uint64_t> sizes{big.size(), html.size(), 0};
  const std::vector<std::uint32_t> lens{1, 18, 5};
  const std::size_t cap = zip_bound(sizes, lens);
  std::size_t want = 22 + 76;
  for (std::size_t i = 0; i < 3; ++i) want += 30 + 46 + 2 * lens[i] + compress_bound(static_cast<std::size_t>(sizes[i]));
  check(cap == want, "zip_bound");
  Bytes file(cap);
  const auto sz = gpu.compress_zip(names, srcs, file);
  check(sz.has_value(), "compress_zip");
  if (!sz.has_value()) return 1;
  file.resize(*sz);
  check(gpu.index().error() != CompressStatus::Success, "no index after a ZIP call");

  const auto ix = zip_read_index(file);
  check(ix.has_value(), "zip_read_index");
  if (!ix.has_value()) return 1;
  check(ix->entries.size() == 3 && !ix->zip64, "the entries");
  for (std::size_t i = 0; i < ix->entries.size(); ++i) {
    const auto& e = ix->entries[i];
    check(e.status == 0 && e.method == 8 && e.usize == sizes[i] && ix->name(file, i) == names[i] && e.out_off % 16 == 0, "an entry's row");
    // every body is a raw stream of its own: the serial decoder reads it
    Bytes part(sizes[i] ? sizes[i] : 1);
    const auto body = std::span{file}.subspan(static_cast<std::size_t>(e.data_off), static_cast<std::size_t>(e.csize));
    const auto st = decompress(body, std::span{part}.first(static_cast<std::size_t>(sizes[i])));
    check(st == DecompressStatus::Success && std::memcmp(part.data(), srcs[i].data(), srcs[i].size()) == 0, "a body alone");
  }
  // all entries, then a subset in another order
  std::vector<Bytes> outs{Bytes(big.size()), Bytes(html.size()), Bytes(1)};
  std::vector<std::span<std::byte>> dsts{outs[0], outs[1], std::span{outs[2]}.first(0)};
  std::vector<std::uint32_t> st(3, 99);
  check(gpu.decompress_zip(file, ix->entries, dsts, st) == CompressStatus::Success, "decompress_zip");
  check(st == std::vector<std::uint32_t>{0, 0, 0} && outs[0] == big && outs[1] == html, "the entries' bytes");
  const std::vector<sfh_zip_entry> pick{ix->entries[1], ix->entries[0]};
  std::vector<Bytes> outs2{Bytes(html.size()), Bytes(big.size())};
  std::vector<std::span<std::byte>> dsts2{outs2[0], outs2[1]};
  std::vector<std::uint32_t> st2(2, 99);
  check(gpu.decompress_zip(file, pick, dsts2, st2) == CompressStatus::Success && st2 == std::vector<std::uint32_t>{0, 0} &&
            outs2[0] == html && outs2[1] == big, "a subset in another order");
  // a flipped body byte: that entry alone ends in a status
  Bytes bad = file;
  bad[static_cast<std::size_t>(ix->entries[1].data_off + ix->entries[1].csize / 2)] ^= std::byte{0x10};
  outs[0].assign(big.size(), std::byte{0});
  st.assign(3, 99);
  check(gpu.decompress_zip(bad, ix->entries, dsts, st) == CompressStatus::Success && st[0] == 0 && st[1] != 0 && st[2] == 0 && outs[0] == big,
        "a flipped byte");
  // the options and names the writer refuses
  compress_options opt;
  opt.container = Container::Gzip;
  check(gpu.compress_zip(names, srcs, file, opt).error() == CompressStatus::InvalidArgument, "container must be Raw");
  const std::vector<std::string_view> noname{"a", "", "c"};
  Bytes again(cap);
  check(gpu.compress_zip(noname, srcs, again).error() == CompressStatus::InvalidArgument, "an empty name");
  check(gpu.compress_zip(names, srcs, std::span{again}.first(cap - 1)).error() == CompressStatus::DstTooSmall, "capacity");
  const auto e = gpu.compress_zip({}, {}, again);
  check(e.has_value() && *e == 22, "no items: the empty archive");
  check(!zip_read_index(std::span{file}.first(file.size() - 1)).has_value(), "zip_read_index on a truncated file");

  // an archive another tool wrote
  if (argc > 2) {
    const std::string path = argv[2];
    const auto foreign = read_file(path);
    const auto fx = zip_read_index(foreign);
    check(fx.has_value() && !fx->entries.empty(), "a foreign archive's index");
    if (fx.has_value()) {
      const std::size_t k = fx->entries.size();
      std::vector<Bytes> fo(k);
      std::vector<std::span<std::byte>> fd(k);
      for (std::size_t i = 0; i < k; ++i) {
        fo[i].resize(static_cast<std::size_t>(fx->entries[i].usize));
        fd[i] = fo[i];
      }
      std::vector<std::uint32_t> fs(k, 99);
      check(gpu.decompress_zip(foreign, fx->entries, fd, fs) == CompressStatus::Success, "a foreign archive");
      for (std::size_t i = 0; i < k; ++i) check(fs[i] == 0 && fo[i] == read_file(path + "." + std::to_string(i)), "a foreign entry");
    }
  }
  std::printf(fail ? "%d checks failed\n" : "zip ok (%d failures)\n", fail);
  return fail ? 1 : 0;
}
