// GPU test of the C++23 seekable-gzip members: compressor::compress with Container::Dictzip writes a gzip file the serial
// decoder reads as Container::Gzip (and as Container::Dictzip); starflate::dz_read_index() gives the compressor's own index from
// the file alone; compressor::decompress_dz() and decompress_dz_range() read the file and parts of it given nothing but its
// bytes; a plain gzip file has no such index.  argv[1] = tests/golden.
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
  Bytes in;  // 5 segments and a few bytes
  while (in.size() < 5 * 32768 + 77) in.insert(in.end(), html.begin(), html.end());
  in.resize(5 * 32768 + 77);
  const std::size_t n = in.size();
  int fail = 0;
  const auto check = [&](bool ok, const char* what) {
    if (!ok) {
      std::printf("failed: %s\n", what);
      ++fail;
    }
  };
  compress_options opt;
  opt.container = Container::Dictzip;
  check(compress_bound(n, 0, Container::Dictzip) == compress_bound(n) + 12 + 2 * 6, "compress_bound for the container");
  check(compress_bound(n, 65536, Container::Dictzip) == 0, "compress_bound refuses block_bytes 65536");
  Bytes file(compress_bound(n, 0, Container::Dictzip));
  const auto sz = gpu.compress(in, file, opt);
  if (!sz) {
    std::printf("compress failed: %d\n", static_cast<int>(sz.error()));
    return 1;
  }
  file.resize(*sz);
  const auto own = gpu.index(false);
  const auto ix = dz_read_index(file);
  check(own && ix && ix->offsets == own->offsets && ix->total_bytes == n && ix->block_bytes == 32768 && ix->segments() == 6,
        "dz_read_index gives the compressor's index");
  // the serial decoder: an ordinary gzip file
  Bytes back(n, std::byte{0});
  check(starflate::decompress(file, back, Container::Gzip) == DecompressStatus::Success && back == in, "serial gzip decode");
  back.assign(n, std::byte{0});
  check(starflate::decompress(file, back, Container::Dictzip) == DecompressStatus::Success && back == in, "serial decode as Dictzip");
  // the GPU, with nothing but the file
  back.assign(n + 10, std::byte{0});
  std::size_t produced = 0;
  check(gpu.decompress_dz(file, back, &produced) == DecompressStatus::Success && produced == n &&
            std::memcmp(back.data(), in.data(), n) == 0,
        "decompress_dz");
  if (ix) {
    back.assign(n, std::byte{0});
    check(gpu.decompress(file, back, *ix) == DecompressStatus::Success && back == in, "decompress with the index read back");
  }
  for (const std::uint64_t off : {std::uint64_t{0}, std::uint64_t{32767}, std::uint64_t{3 * 32768 - 5}, std::uint64_t{n - 9}}) {
    Bytes part(9 + (off % 3) * 20000, std::byte{0x5A});
    if (off + part.size() > n) part.resize(n - off);
    check(gpu.decompress_dz_range(file, part, off) == DecompressStatus::Success && std::memcmp(part.data(), in.data() + off, part.size()) == 0,
          "decompress_dz_range");
  }
  Bytes part(4);
  check(gpu.decompress_dz_range(file, part, n - 3) == DecompressStatus::Error, "a range behind the end is refused");
  // a damaged CRC: Error from the GPU and from the serial decoder it falls back to
  Bytes bad = file;
  bad[bad.size() - 8] ^= std::byte{1};
  back.assign(n, std::byte{0});
  check(gpu.decompress_dz(bad, back) == DecompressStatus::Error, "a damaged CRC");
  // a plain gzip file: no index in it; decompress_dz still decodes it
  opt.container = Container::Gzip;
  Bytes plain(compress_bound(n));
  const auto psz = gpu.compress(in, plain, opt);
  if (!psz) return 1;
  plain.resize(*psz);
  const auto none = dz_read_index(plain);
  check(!none && none.error() == CompressStatus::NotIndexable, "a plain gzip file is NotIndexable");
  back.assign(n, std::byte{0});
  check(gpu.decompress_dz(plain, back) == DecompressStatus::Success && back == in, "decompress_dz falls back for a plain gzip file");
  check(gpu.decompress_dz_range(plain, part, 0) == DecompressStatus::Error, "no ranges of a plain gzip file");
  // the batched call refuses the container
  opt.container = Container::Dictzip;
  const std::span<const std::byte> srcs[1] = {in};
  const std::span<std::byte> dsts[1] = {file};
  std::size_t sizes[1] = {0};
  file.resize(compress_bound(n, 0, Container::Dictzip));
  const auto b = gpu.compress_batch(srcs, dsts, sizes, opt);
  check(!b && b.error() == CompressStatus::InvalidArgument, "compress_batch refuses Container::Dictzip");
  std::printf("dictzip: %d failed\n", fail);
  return fail ? 1 : 0;
}
