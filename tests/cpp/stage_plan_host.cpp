// Host shim for tests/test_stage_plan_host.py: the staging loops of sf_stage_plan.h (what the batched host-buffer entry points
// run between the callers' buffers and the device staging) with a host buffer standing in for the device and a pinned buffer
// of `piece` bytes.  TEST INFRASTRUCTURE ONLY.
#include "../../starflate_amd/csrc/sf_stage_plan.h"

#include <vector>

extern "C" {

// items[item_off[i], +len[i]) -> dev[off[i], +len[i]) through pieces of [0, total); copied[k] = the k-th transfer's p0 and
// size (2 words each, room for `cap` transfers) -> the number of transfers
uint64_t sfg_pack_up(uint64_t piece, uint64_t count, const uint8_t* items, const uint64_t* item_off, const uint64_t* len,
                     const uint64_t* off, uint64_t total, uint8_t* dev, uint64_t* copied, uint64_t cap) {
  std::vector<uint8_t> stage(piece, 0xEE);
  std::vector<const void*> src(count);
  for (uint64_t i = 0; i < count; ++i) src[i] = items + item_off[i];
  uint64_t k = 0;
  sf::stage::pack_up(stage.data(), piece, src.data(), len, off, count, total, [&](uint64_t p0, uint64_t n) -> int {
    memcpy(dev + p0, stage.data(), n);
    if (k < cap) copied[2 * k] = p0, copied[2 * k + 1] = n;
    ++k;
    return 0;
  });
  return k;
}

// dev[off[i], +len[i]) -> out[item_off[i], +len[i]) for every i with len[i] != 0; copied as above
uint64_t sfg_unpack_down(uint64_t piece, uint64_t count, const uint8_t* dev, const uint64_t* len, const uint64_t* off,
                         uint64_t total, uint8_t* out, const uint64_t* item_off, uint64_t* copied, uint64_t cap) {
  std::vector<uint8_t> stage(piece, 0xEE);
  std::vector<void*> dst(count);
  for (uint64_t i = 0; i < count; ++i) dst[i] = out + item_off[i];
  uint64_t k = 0;
  sf::stage::unpack_down(stage.data(), piece, dst.data(), len, off, count, total, [&](uint64_t p0, uint64_t n) -> int {
    memcpy(stage.data(), dev + p0, n);
    if (k < cap) copied[2 * k] = p0, copied[2 * k + 1] = n;
    ++k;
    return 0;
  });
  return k;
}

// a transfer that fails: the loops stop and hand its code on -> that code
int sfg_failing_transfer(uint64_t piece, const uint8_t* item, uint64_t n, uint64_t fail_at, uint64_t* transfers) {
  std::vector<uint8_t> stage(piece);
  const void* src[1] = {item};
  const uint64_t len[1] = {n}, off[1] = {0};
  *transfers = 0;
  return sf::stage::pack_up(stage.data(), piece, src, len, off, 1, n, [&](uint64_t, uint64_t) -> int {
    return ++*transfers == fail_at ? -7 : 0;
  });
}
}
