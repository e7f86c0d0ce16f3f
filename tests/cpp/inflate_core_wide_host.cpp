// decode_segment (starflate_amd/csrc/sf_inflate_core.h) on segments above 32 KiB of output -- the wide rows of the indexed
// decoder, a BGZF member of up to 65536 bytes -- and the wide-row arithmetic of sf_bgzf_plan.h, compiled for the host.
// tests/test_inflate_core_wide_host.py runs cases made with Python's zlib and tests/deflate_writer.py through sfiw_decode (a
// shared library) and through main() below, built with AddressSanitizer + UBSan: every body in a heap allocation of its size
// rounded up to a dword (the bit reader loads aligned dwords of the stream and never one that holds no byte of it), the
// tokens in one of exactly out_n entries -- a row holds a token per output byte -- and the output in one of exactly out_n bytes.
#include "../../starflate_amd/csrc/sf_bgzf_plan.h"
#include "../../starflate_amd/csrc/sf_inflate_core.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

// the body [0, n) decoded as one segment of out_n bytes into out[0 .. out_n).  -> the decoder's status; 100: a token the byte
// stage would refuse; 101: the tokens expand to other than out_n bytes
unsigned decode(const uint8_t* body, uint64_t n, uint32_t out_n, uint8_t* out) {
  alignas(16) unsigned char mem[sf::inflate::LaneLayout::kBytes + 12];
  memset(mem, 0xA5, sizeof mem);
  uint8_t* src = (uint8_t*)malloc(n ? (size_t)((n + 3) & ~3ull) : 4);
  uint32_t* tokens = (uint32_t*)aligned_alloc(16, out_n ? ((size_t)out_n * 4 + 15) & ~(size_t)15 : 16);  // (whole 16-byte groups)
  if (!src || !tokens) abort();
  memcpy(src, body, (size_t)n);
  const sf::inflate::SegmentResult r = sf::inflate::decode_segment(src, n, 0, n, out_n, tokens, mem);
  unsigned st = r.status;
  if (st == sf::inflate::kOk && r.raw) {
    if (r.raw_off + out_n > n) st = 100;
    else memcpy(out, src + r.raw_off, out_n);
  } else if (st == sf::inflate::kOk) {
    if (r.ntok > out_n) st = 100;
    uint32_t pos = 0;
    for (uint32_t i = 0; i < r.ntok && st == sf::inflate::kOk; ++i) {
      const uint32_t t = tokens[i];
      if (t & 0x80000000u) {
        const uint32_t len = ((t >> 16) & 0xFF) + 3, dist = (t & 0x7FFF) + 1;
        if (dist > pos || len > out_n - pos) st = 100;
        else
          for (uint32_t k = 0; k < len; ++k, ++pos) out[pos] = out[pos - dist];
      } else if (pos >= out_n || t > 255) {
        st = 100;
      } else {
        out[pos++] = (uint8_t)t;
      }
    }
    if (st == sf::inflate::kOk && pos != out_n) st = 101;
  }
  free(tokens);
  free(src);
  return st;
}

}  // namespace

extern "C" {
unsigned sfiw_decode(const uint8_t* body, uint64_t n, uint32_t out_n, uint8_t* out) { return decode(body, n, out_n, out); }
uint32_t sfiw_wide_batch(uint32_t batch_chunks) { return sf::bgzf::wide_batch(batch_chunks); }
uint64_t sfiw_checksum_rows(uint64_t members, int wide) { return sf::bgzf::checksum_rows(members, wide != 0); }
}

// main(cases file): case after case, each u64 body bytes, u32 out_n, u32 the status wanted, the body, and -- status 0 -- the
// out_n bytes wanted.  Prints "status same" per case (same: the output is the wanted one), then the count.
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  size_t cases = 0;
  for (;;) {
    uint64_t n = 0;
    uint32_t out_n = 0, want = 0;
    if (fread(&n, sizeof n, 1, f) != 1) break;
    if (fread(&out_n, sizeof out_n, 1, f) != 1 || fread(&want, sizeof want, 1, f) != 1) return 2;
    uint8_t* body = (uint8_t*)malloc(n ? (size_t)n : 1);
    uint8_t* expect = (uint8_t*)malloc(out_n ? out_n : 1);
    uint8_t* out = (uint8_t*)malloc(out_n ? out_n : 1);  // exactly the output
    if (!body || !expect || !out || (n && fread(body, 1, (size_t)n, f) != n)) return 2;
    if (want == 0 && out_n && fread(expect, 1, out_n, f) != out_n) return 2;
    const unsigned st = decode(body, n, out_n, out);
    printf("%u %d\n", st, (st == 0 && want == 0 && memcmp(out, expect, out_n) == 0) ? 1 : 0);
    free(out);
    free(expect);
    free(body);
    ++cases;
  }
  fclose(f);
  printf("%zu cases\n", cases);
  return 0;
}
