// GPU test of the C++23 one-call read path: compressor::decompress(src, dst, Container) -- the index recovered on the GPU, the
// serial decoder behind it -- must give, on every case, the status and bytes of container.hpp's decompress(src, dst,
// Container); compressor::recover_index() must give the writer's index on intact streams of this library.
// argv[1] = a directory holding cases.txt ("<file> <container 0|1|2> <dst_n> <index file or ->" per line) and the files.
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

auto main(int argc, char** argv) -> int {
  using namespace starflate;
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  compressor gpu{0};
  std::ifstream list{dir + "/cases.txt"};
  std::string line;
  int failed = 0, cases = 0, gpu_ok = 0;
  while (std::getline(list, line)) {
    std::istringstream ls{line};
    std::string name, ixname;
    unsigned kind = 0;
    std::size_t n = 0;
    ls >> name >> kind >> n >> ixname;
    const auto src = read_file(dir + "/" + name);
    const auto container = static_cast<Container>(kind);
    std::vector<std::byte> a(n), b(n);
    const auto got = gpu.decompress(src, a, container);
    const auto want = decompress(src, b, container);
    ++cases;
    if (got != want || (want == DecompressStatus::Success && a != b)) {
      std::printf("FAIL %s: status %d, serial %d\n", name.c_str(), static_cast<int>(got), static_cast<int>(want));
      ++failed;
    }
    if (ixname != "-") {
      const auto raw = read_file(dir + "/" + ixname);
      std::vector<std::uint64_t> ix(raw.size() / 8);
      std::memcpy(ix.data(), raw.data(), raw.size());
      const auto rec = gpu.recover_index(src, n, container);
      if (!rec || rec->offsets != ix) {
        std::printf("FAIL %s: recovered index\n", name.c_str());
        ++failed;
      } else {
        ++gpu_ok;
      }
    }
  }
  std::printf("%d cases, %d indexes recovered, %d failed\n", cases, gpu_ok, failed);
  return failed ? 1 : 0;
}
