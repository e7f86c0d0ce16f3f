// any_plan_host.cpp -- starflate_amd/csrc/sf_any_plan.h (the cut of an index-free batch decode into launch batches) as a
// stand-alone host program: the named cases of its rule and random calls against a plain model.  Prints "N checks, M failed";
// built by tests/test_any_plan_host.py with every warning an error, plain and under AddressSanitizer + UBSan.
#include "../../starflate_amd/csrc/sf_any_plan.h"

#include <stdio.h>

#include <random>
#include <utility>
#include <vector>

namespace {

using sf::aplan::Batch;
using sf::aplan::Plan;
constexpr uint64_t SEG = sf::aplan::kSegBytes;

int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++g_checks;                                                  \
    if (!(cond)) {                                               \
      ++g_failed;                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
    }                                                            \
  } while (0)

uint32_t nseg_of(uint64_t n) { return n ? (uint32_t)((n + SEG - 1) / SEG) : 1u; }

Plan plan(const std::vector<uint64_t>& out_n, const std::vector<uint8_t>* take, uint32_t cap) {
  Plan P;
  sf::aplan::plan_batches(out_n.size(), out_n.data(), take ? take->data() : nullptr, cap, P);
  return P;
}

// the properties of the rule, for any call
void check(const Plan& P, const std::vector<uint64_t>& out_n, const std::vector<uint8_t>* take, uint32_t cap) {
  const size_t count = out_n.size();
  uint64_t segs = 0, items = 0;
  for (size_t i = 0; i < count; ++i)
    if (!take || (*take)[i]) {
      segs += nseg_of(out_n[i]);
      ++items;
    }
  CHECK(P.nseg == segs && P.nitems == items);  // totals
  size_t item_at = 0;
  uint32_t row_at = 0, widest = 0;
  uint64_t seen_items = 0;
  for (const Batch& b : P.batches) {
    // item order and rows preserved: the batches follow each other in both
    CHECK(b.item0 >= item_at && b.item0 < b.item1 && b.item1 <= count);
    CHECK(b.row0 == row_at && b.nseg > 0 && b.nitems > 0);
    for (size_t i = item_at; i < b.item0 && i < count; ++i) CHECK(take && !(*take)[i]);  // only idle items between batches
    uint64_t n = 0, k = 0;
    for (size_t i = b.item0; i < b.item1 && i < count; ++i)
      if (!take || (*take)[i]) {
        n += nseg_of(out_n[i]);  // whole items only
        ++k;
      }
    CHECK(n == b.nseg && k == b.nitems);
    CHECK(b.nseg <= cap || b.nitems == 1);  // at most cap segments, or one larger item alone
    CHECK(!take || (*take)[b.item0]);       // a batch is named by its first item that takes part
    if (b.nseg > widest) widest = b.nseg;
    item_at = b.item1;
    row_at += b.nseg;
    seen_items += b.nitems;
  }
  for (size_t i = item_at; i < count; ++i) CHECK(take && !(*take)[i]);
  CHECK(row_at == P.nseg && seen_items == P.nitems && widest == P.widest);
  // greedy: two neighbouring batches would not have fitted into one
  for (size_t j = 0; j + 1 < P.batches.size(); ++j)
    CHECK((uint64_t)P.batches[j].nseg + nseg_of(out_n[P.batches[j + 1].item0]) > cap);
}

std::vector<std::pair<uint32_t, uint32_t>> shape(const Plan& P) {  // {segments, items} per batch
  std::vector<std::pair<uint32_t, uint32_t>> v;
  for (const Batch& b : P.batches) v.push_back({b.nseg, b.nitems});
  return v;
}
using Shape = std::vector<std::pair<uint32_t, uint32_t>>;

}  // namespace

int main() {
  {  // an item exactly at the cap: a batch of its own, full, and not "larger than the cap"
    const std::vector<uint64_t> n{SEG, 4 * SEG, SEG};
    const Plan P = plan(n, nullptr, 4);
    check(P, n, nullptr, 4);
    CHECK((shape(P) == Shape{{1, 1}, {4, 1}, {1, 1}}));
    const std::vector<uint64_t> m{4 * SEG, 2 * SEG, 2 * SEG, SEG};
    const Plan Q = plan(m, nullptr, 4);
    check(Q, m, nullptr, 4);
    CHECK((shape(Q) == Shape{{4, 1}, {4, 2}, {1, 1}}));
  }
  {  // one segment over the cap: alone and whole, and the item behind it opens a new batch
    const std::vector<uint64_t> n{SEG, 4 * SEG + 1, SEG, SEG};
    const Plan P = plan(n, nullptr, 4);
    check(P, n, nullptr, 4);
    CHECK((shape(P) == Shape{{1, 1}, {5, 1}, {2, 2}}));
    CHECK(P.widest == 5 && P.batches[1].item0 == 1 && P.batches[1].item1 == 2 && P.batches[2].item0 == 2);
  }
  {  // empty items: one segment each, which decodes to nothing
    const std::vector<uint64_t> n{0, 0, 0, 3 * SEG, 0, 0};
    const Plan P = plan(n, nullptr, 4);
    check(P, n, nullptr, 4);
    CHECK((shape(P) == Shape{{3, 3}, {4, 2}, {1, 1}}));
    const std::vector<uint64_t> none;
    const Plan E = plan(none, nullptr, 4);
    CHECK(E.batches.empty() && E.nseg == 0 && E.widest == 0);
  }
  {  // a cap of 1: every item alone
    const std::vector<uint64_t> n{1, 0, SEG + 1, SEG, 7 * SEG};
    const Plan P = plan(n, nullptr, 1);
    check(P, n, nullptr, 1);
    CHECK((shape(P) == Shape{{1, 1}, {1, 1}, {2, 1}, {1, 1}, {7, 1}}));
  }
  {  // items that take no part have no rows, wherever they stand
    const std::vector<uint64_t> n{2 * SEG, 9 * SEG, SEG, 0, 2 * SEG, SEG};
    const std::vector<uint8_t> take{1, 0, 1, 0, 1, 0};
    const Plan P = plan(n, &take, 4);
    check(P, n, &take, 4);
    CHECK((shape(P) == Shape{{3, 2}, {2, 1}}));
    const std::vector<uint8_t> nobody(n.size(), 0);
    const Plan N = plan(n, &nobody, 4);
    check(N, n, &nobody, 4);
    CHECK(N.batches.empty() && N.nseg == 0);
  }
  // random calls against the properties
  std::mt19937_64 rng(20240);
  const uint64_t sizes[] = {0, 1, SEG - 1, SEG, SEG + 1, 3 * SEG, 4 * SEG, 4 * SEG + 1, 8 * SEG, 9 * SEG + 777, 70 * SEG + 1};
  const uint32_t caps[] = {1, 2, 3, 4, 8, 32768};
  for (int round = 0; round < 400; ++round) {
    const size_t count = (size_t)(rng() % 14);
    std::vector<uint64_t> n(count);
    std::vector<uint8_t> take(count);
    for (size_t i = 0; i < count; ++i) {
      n[i] = rng() % 2 ? sizes[rng() % (sizeof sizes / sizeof *sizes)] : rng() % (12 * SEG);
      take[i] = rng() % 4 != 0;
    }
    const uint32_t cap = caps[rng() % (sizeof caps / sizeof *caps)];
    check(plan(n, nullptr, cap), n, nullptr, cap);
    check(plan(n, &take, cap), n, &take, cap);
  }
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
