// GPU test of the C++23 batched read path: compressor::decompress_batch(srcs, dsts, Container, statuses) -- every index
// recovered on the GPU in one call, the serial decoder behind the items the GPU did not decode -- must give, for every item,
// the status and bytes of container.hpp's decompress(src, dst, Container); compressor::recover_index_batch() must give the
// writer's index on intact streams of this library and say which items are not indexable.
// argv[1] = a directory holding cases.txt ("<file> <container 0|1|2> <dst_n> <index file or ->" per line) and the files; the
// cases of one container, in file order, are one batch.
#include "starflate/compress.hpp"
#include "starflate/container.hpp"
#include "starflate/decompress.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <span>
#include <sstream>
#include <string>
#include <vector>

static auto read_file(const std::string& path) -> std::vector<std::byte> {
  std::ifstream f{path, std::ios::binary};
  std::vector<char> c((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<std::byte> b(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) b[i] = static_cast<std::byte>(c[i]);
  return b;
}

struct item {
  std::string name, ixname;
  std::vector<std::byte> src, got, want;
};

auto main(int argc, char** argv) -> int {
  using namespace starflate;
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  compressor gpu{0};
  std::vector<item> items[3];
  std::ifstream list{dir + "/cases.txt"};
  std::string line;
  while (std::getline(list, line)) {
    std::istringstream ls{line};
    item it;
    unsigned kind = 0;
    std::size_t n = 0;
    ls >> it.name >> kind >> n >> it.ixname;
    if (kind > 2) return 2;
    it.src = read_file(dir + "/" + it.name);
    it.got.assign(n, std::byte{0xA5});
    it.want.assign(n, std::byte{0xA5});
    items[kind].push_back(std::move(it));
  }
  int failed = 0, cases = 0, gpu_ok = 0, not_indexable = 0;
  for (unsigned kind = 0; kind < 3; ++kind) {
    auto& v = items[kind];
    const auto container = static_cast<Container>(kind);
    std::vector<std::span<const std::byte>> srcs;
    std::vector<std::span<std::byte>> dsts;
    std::vector<std::size_t> sizes;
    for (auto& it : v) {
      srcs.emplace_back(it.src);
      dsts.emplace_back(it.got);
      sizes.push_back(it.got.size());
    }
    std::vector<DecompressStatus> st(v.size(), DecompressStatus::Error);
    if (gpu.decompress_batch(srcs, dsts, container, st) != CompressStatus::Success) {
      std::printf("FAIL container %u: the call was refused\n", kind);
      ++failed;
      continue;
    }
    std::vector<bool> indexable;
    const auto rec = gpu.recover_index_batch(srcs, sizes, container, &indexable);
    if (!rec || rec->items() != v.size() || indexable.size() != v.size()) {
      std::printf("FAIL container %u: recover_index_batch\n", kind);
      ++failed;
      continue;
    }
    for (std::size_t i = 0; i < v.size(); ++i) {
      const auto want = decompress(v[i].src, v[i].want, container);
      ++cases;
      if (st[i] != want || (want == DecompressStatus::Success && v[i].got != v[i].want)) {
        std::printf("FAIL %s: status %d, serial %d\n", v[i].name.c_str(), static_cast<int>(st[i]), static_cast<int>(want));
        ++failed;
      }
      if (!indexable[i]) ++not_indexable;
      if (v[i].ixname == "-") continue;
      const auto raw = read_file(dir + "/" + v[i].ixname);
      std::vector<std::uint64_t> ix(raw.size() / 8);
      std::memcpy(ix.data(), raw.data(), raw.size());
      const std::vector<std::uint64_t> mine(rec->offsets.begin() + static_cast<std::ptrdiff_t>(rec->first[i]),
                                            rec->offsets.begin() + static_cast<std::ptrdiff_t>(rec->first[i + 1]));
      if (!indexable[i] || mine != ix || rec->block_bytes[i] != 0 || !rec->regions.empty()) {
        std::printf("FAIL %s: recovered index\n", v[i].name.c_str());
        ++failed;
      } else {
        ++gpu_ok;
      }
    }
  }
  std::printf("%d cases, %d indexes recovered, %d not indexable, %d failed\n", cases, gpu_ok, not_indexable, failed);
  return failed ? 1 : 0;
}
