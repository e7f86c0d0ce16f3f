// GPU test of the C++23 batch decoder: compressor::batch_index() and compressor::decompress_batch() over items of mixed
// sizes, raw, zlib and gzip, intact and damaged.  Every item's status is compared with the host decoder's,
// starflate::decompress(src, dst, Container) (container.hpp), and every intact item's bytes with the input.
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

static auto read_file(const std::string& path) -> std::vector<std::byte> {
  std::ifstream f{path, std::ios::binary};
  std::vector<char> c((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<std::byte> b(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) b[i] = static_cast<std::byte>(c[i]);
  return b;
}

using Bytes = std::vector<std::byte>;

// decode `streams` in one batch call (ix: nullptr or the batch index) and compare with the host decoder item by item
static auto check(starflate::compressor& gpu, const std::vector<Bytes>& streams, const std::vector<std::size_t>& sizes,
                  const starflate::batch_stream_index* ix, starflate::Container kind, const std::vector<Bytes>* want,
                  const char* what) -> int {
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
  const auto rc = gpu.decompress_batch(srcs, dsts, ix, kind, st);
  if (rc != CompressStatus::Success) {
    std::printf("%s: decompress_batch refused: %d\n", what, static_cast<int>(rc));
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
    if (want != nullptr && (st[i] != DecompressStatus::Success || out[i] != (*want)[i])) {
      std::printf("%s, item %zu (container %d): not the input back\n", what, i, static_cast<int>(kind));
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
  Bytes big;  // 300 KiB of the page over and over, then a few bytes of noise
  while (big.size() < 300 * 1024) big.insert(big.end(), html.begin(), html.end());
  std::uint32_t x = 12345;
  for (int i = 0; i < 777; ++i) big.push_back(static_cast<std::byte>((x = x * 1103515245U + 12345U) >> 24));
  items.push_back(big);
  std::vector<std::size_t> sizes;
  for (const auto& a : items) sizes.push_back(a.size());
  int fail = 0;
  for (const auto kind : {Container::Raw, Container::Zlib, Container::Gzip}) {
    compress_options opt;
    opt.container = kind;
    std::vector<Bytes> out;
    std::vector<std::span<const std::byte>> srcs;
    std::vector<std::span<std::byte>> dsts;
    for (const auto& in : items) out.emplace_back(compress_bound(in.size()));
    for (std::size_t i = 0; i < items.size(); ++i) {
      srcs.emplace_back(items[i]);
      dsts.emplace_back(out[i]);
    }
    std::vector<std::size_t> n(items.size());
    if (!gpu.compress_batch(srcs, dsts, n, opt)) {
      std::printf("compress_batch failed\n");
      return 1;
    }
    const auto ix = gpu.batch_index();
    const auto ix_plain = gpu.batch_index(false);
    if (!ix || !ix_plain || ix->items() != items.size()) {
      std::printf("batch_index failed\n");
      return 1;
    }
    std::vector<Bytes> streams;
    for (std::size_t i = 0; i < items.size(); ++i) streams.emplace_back(out[i].begin(), out[i].begin() + static_cast<std::ptrdiff_t>(n[i]));
    fail += check(gpu, streams, sizes, &*ix, kind, &items, "intact, sub-index");
    fail += check(gpu, streams, sizes, &*ix_plain, kind, &items, "intact, index");
    if (kind == Container::Raw) continue;
    // damaged wrapped items, every case on its own copy of the batch (the other items stay intact)
    const std::size_t hdr = kind == Container::Zlib ? 2 : 10, tr = kind == Container::Zlib ? 4 : 8;
    for (int c = 0; c < 8; ++c) {
      std::vector<Bytes> d = streams;
      std::vector<std::size_t> ds = sizes;
      for (std::size_t i = 1; i < d.size(); ++i) {  // (item 0 stays intact throughout)
        Bytes& s = d[i];
        switch (c) {
          case 0: s[0] ^= std::byte{0x01}; break;                                   // a header byte
          case 1: s[s.size() - tr] ^= std::byte{0x40}; break;                       // a checksum byte
          case 2: s[hdr] |= std::byte{0x06}; break;                                 // BTYPE 3: the body fails
          case 3: s[hdr] |= std::byte{0x06}; s[s.size() - tr] ^= std::byte{0x40}; break;  // ... and its checksum with it
          case 4: s.resize(kind == Container::Zlib ? 5 : 17); break;                // shorter than the wrapper
          case 5: ds[i] += 1; break;                                                // one byte more expected than written
          case 6: if (kind == Container::Gzip) s[s.size() - 4] = static_cast<std::byte>(std::to_integer<unsigned>(s[s.size() - 4]) + 1); break;  // ISIZE + 1
          case 7: if (kind == Container::Gzip) s[s.size() - 4] = static_cast<std::byte>(std::to_integer<unsigned>(s[s.size() - 4]) - 1); break;  // ISIZE - 1
        }
      }
      const std::string what = "damage case " + std::to_string(c);
      if (c == 5) {
        // other output sizes: the index no longer fits them, so the small items go index-free
        std::vector<Bytes> small;
        std::vector<std::size_t> ss;
        for (std::size_t i = 0; i < d.size(); ++i)
          if (ds[i] <= SFH_SEGMENT_BYTES) {
            small.push_back(d[i]);
            ss.push_back(ds[i]);
          }
        fail += check(gpu, small, ss, nullptr, kind, nullptr, what.c_str());
        continue;
      }
      fail += check(gpu, d, ds, &*ix, kind, nullptr, what.c_str());
      fail += check(gpu, d, ds, &*ix_plain, kind, nullptr, what.c_str());
    }
    // the items of at most 32 KiB without any index (each one segment from the header's end to the trailer)
    std::vector<Bytes> small, small_in;
    std::vector<std::size_t> ss;
    for (std::size_t i = 0; i < items.size(); ++i)
      if (sizes[i] <= SFH_SEGMENT_BYTES) {
        small.push_back(streams[i]);
        small_in.push_back(items[i]);
        ss.push_back(sizes[i]);
      }
    fail += check(gpu, small, ss, nullptr, kind, &small_in, "index-free");
  }
  // a refused call: one status slot too few
  {
    const std::vector<std::span<const std::byte>> srcs{html, html};
    Bytes a(10), b(10);
    const std::vector<std::span<std::byte>> dsts{a, b};
    std::vector<DecompressStatus> st(1);
    if (gpu.decompress_batch(srcs, dsts, nullptr, Container::Raw, st) != CompressStatus::InvalidArgument) {
      std::printf("a mismatched status span was not refused\n");
      ++fail;
    }
  }
  std::printf("decompress_batch: %d failed\n", fail);
  return fail ? 1 : 0;
}
