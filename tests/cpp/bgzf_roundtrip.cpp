// GPU test of the C++23 BGZF members: compressor::compress_bgzf writes a file of gzip members the serial decoder reads member
// by member; starflate::bgzf_read_index() finds the members from the file alone; compressor::decompress_bgzf() reads the file
// back, and ends a damaged one in a status.  argv[1] = tests/golden.
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
  Bytes in;  // 5 members and a few bytes
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
  check(bgzf_bound(n) == 6 * (compress_bound(32768) + 26) + 28, "bgzf_bound");
  Bytes file(bgzf_bound(n));
  const auto sz = gpu.compress_bgzf(in, file);
  check(sz.has_value(), "compress_bgzf");
  if (!sz.has_value()) return 1;
  file.resize(*sz);
  check(gpu.index().error() != CompressStatus::Success, "no index after a BGZF call");

  const auto ix = bgzf_read_index(file);
  check(ix.has_value(), "bgzf_read_index");
  if (!ix.has_value()) return 1;
  check(ix->members() == 7 && ix->total_bytes == n && ix->max_isize == 32768 && ix->has_eof, "the members");
  check(ix->member_off.back() == file.size() && ix->out_off[5] == 5 * 32768 && ix->out_off[6] == n, "the offsets");
  // every member is a gzip file of its own 32 KiB: the serial decoder reads it
  for (std::size_t k = 0; k < ix->members(); ++k) {
    const std::size_t on = static_cast<std::size_t>(ix->out_off[k + 1] - ix->out_off[k]);
    Bytes part(on ? on : 1);
    const auto member = std::span{file}.subspan(static_cast<std::size_t>(ix->member_off[k]),
                                                static_cast<std::size_t>(ix->member_off[k + 1] - ix->member_off[k]));
    const auto st = decompress(member, std::span{part}.first(on), Container::Gzip);
    check(st == DecompressStatus::Success && std::memcmp(part.data(), in.data() + ix->out_off[k], on) == 0, "a member alone");
  }
  Bytes back(n);
  std::size_t produced = 0;
  check(gpu.decompress_bgzf(file, back, &produced) == DecompressStatus::Success && produced == n && back == in, "decompress_bgzf");
  Bytes small(n - 1);
  check(gpu.decompress_bgzf(file, small) == DecompressStatus::DstTooSmall, "dst one byte short");
  // a flipped CRC byte, a truncated file: a status, never Success
  Bytes bad = file;
  bad[static_cast<std::size_t>(ix->member_off[3]) - 8] ^= std::byte{0x10};
  check(gpu.decompress_bgzf(bad, back) == DecompressStatus::Error, "a flipped CRC byte");
  check(gpu.decompress_bgzf(std::span{file}.first(file.size() - 5), back) == DecompressStatus::SrcTooSmall, "a truncated file");
  check(!bgzf_read_index(std::span{file}.first(40)).has_value(), "bgzf_read_index on a truncated file");
  // the options the call refuses
  compress_options opt;
  opt.container = Container::Gzip;
  check(gpu.compress_bgzf(in, file, opt).error() == CompressStatus::InvalidArgument, "container must be Raw");
  opt = {};
  opt.block_bytes = 65536;
  Bytes again(bgzf_bound(n));
  check(gpu.compress_bgzf(in, again, opt).error() == CompressStatus::InvalidArgument, "block_bytes 65536");
  // an empty input: the EOF member alone
  const auto e = gpu.compress_bgzf(std::span<const std::byte>{}, again);
  check(e.has_value() && *e == 28, "an empty input");
  std::printf(fail ? "%d checks failed\n" : "bgzf ok (%d failures)\n", fail);
  return fail ? 1 : 0;
}
