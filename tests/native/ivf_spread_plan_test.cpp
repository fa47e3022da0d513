// The chunk schedule of lzk_ivf_spread_rows (csrc/include/ivf_spread_plan.h)
// replayed on the host: a loop per chunk in place of the kernel launch, over
// random shapes, checked against std::stable_sort. Built with
// -fsanitize=address,undefined by tests/unit/test_ivf_spread_plan_native.py:
// the bounce buffer and the column are sized exactly, so a chunk that reads or
// writes out of its bounds is caught, and every write is checked against the
// rows later chunks still have to read.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ivf_spread_plan.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);       \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct Row {
  int list;
  long serial;  // creation order: main rows first, then the tail
};

void one_shape(std::mt19937_64& rng, int shape) {
  auto rnd = [&](long lo, long hi) { return lo + (long)(rng() % (uint64_t)(hi - lo + 1)); };
  const int nlist = (int)rnd(1, 40);
  const long n0 = shape % 17 == 0 ? 0 : rnd(1, 3000);
  static const long kRowBytes[6] = {1, 4, 6, 8, 16, 48};
  const long row_bytes = kRowBytes[rng() % 6];
  const long chunk = shape % 5 == 0 ? std::max<long>(n0, 1) : rnd(1, 300);
  long t = shape % 7 == 0 ? 1 : rnd(1, std::max<long>(2, n0 / 2 + 50));
  // main rows sorted by list, some lists left empty
  std::vector<int> lists(n0);
  for (auto& l : lists) l = (int)rnd(0, nlist - 1) / 2 * 2 % nlist;
  std::sort(lists.begin(), lists.end());
  std::vector<int> tail(t);
  const int mode = shape % 4;  // random lists / all in list 0 / all in the last list / random
  for (auto& l : tail) l = mode == 1 ? 0 : mode == 2 ? nlist - 1 : (int)rnd(0, nlist - 1);
  // the truth: a stable sort of (main, tail) by list
  std::vector<Row> all;
  for (long r = 0; r < n0; ++r) all.push_back({lists[r], r});
  for (long j = 0; j < t; ++j) all.push_back({tail[j], n0 + j});
  std::stable_sort(all.begin(), all.end(), [](const Row& a, const Row& b) { return a.list < b.list; });
  // ins[l] = tail rows whose list is < l; old_off = CSR of the main rows
  std::vector<long> ins(nlist + 1, 0), off(nlist + 1, 0);
  for (int l : tail) ins[l + 1] += 1;
  for (int l = 0; l < nlist; ++l) ins[l + 1] += ins[l];
  for (int l : lists) off[l + 1] += 1;
  for (int l = 0; l < nlist; ++l) off[l + 1] += off[l];
  // the column: row r holds its serial in every byte position (mod 251) + the byte index
  const long cap = n0 + t;
  auto byte_of = [&](long serial, long b) { return (uint8_t)((serial * 31 + b * 7) % 251); };
  std::vector<uint8_t> col((size_t)(cap * row_bytes), 0xEE);
  for (long r = 0; r < n0; ++r)
    for (long b = 0; b < row_bytes; ++b) col[(size_t)(r * row_bytes + b)] = byte_of(r, b);
  long first = n0;
  for (long r = 0; r < n0; ++r)
    if (ins[lists[r]] > 0) {
      first = r;
      break;
    }
  if (shape % 3 == 0) first = std::min<long>(first, rnd(0, std::max<long>(first, 0)));  // also from below
  std::vector<long> bounds;
  for (long c0 = first; c0 < n0; c0 += chunk) bounds.push_back(ins[lists[c0]]);
  bounds.push_back(n0 > 0 ? ins[lists[n0 - 1]] : 0);
  const long bounce_rows = std::min(chunk, std::max<long>(n0 - first, 0));
  std::vector<uint8_t> bounce((size_t)(bounce_rows * row_bytes));
  long stats[3];
  long lowest = n0;  // the chunks must come in descending order
  long emitted = 0;
  auto emit = [&](const IvfSpreadChunk& c) {
    ++emitted;
    CHECK(c.c1 <= lowest && c.c0 < c.c1);
    lowest = c.c0;
    const uint8_t* src = col.data();
    long row0 = 0;
    if (!c.direct) {
      CHECK((c.c1 - c.c0) * row_bytes <= (long)bounce.size());
      std::memcpy(bounce.data(), col.data() + c.c0 * row_bytes, (size_t)((c.c1 - c.c0) * row_bytes));
      src = bounce.data();
      row0 = c.c0;
    }
    for (long r = c.c0; r < c.c1; ++r) {
      const long sh = ins[lists[r]];
      CHECK(sh >= c.lo && sh <= c.hi);
      const long d = r + sh;
      CHECK(d >= c.c0 && d < cap);         // never onto a row a later chunk reads
      if (c.direct) CHECK(d >= c.c1);      // never onto a row of the same launch
      std::memcpy(col.data() + d * row_bytes, src + (r - row0) * row_bytes, (size_t)row_bytes);
    }
  };
  const int rc = ivf_spread_plan(n0, first, chunk, bounds.data(), cap, row_bytes, (long)bounce.size(), true, stats,
                                 emit);
  CHECK(rc == 0);
  CHECK(stats[1] + stats[2] == emitted);
  if (mode == 2) CHECK(emitted == 0);  // all in the last list: nothing moves
  // the tail drops into the gaps: behind the old rows of its list, in creation order
  std::vector<long> next(nlist, 0);
  for (long j = 0; j < t; ++j) {
    const int l = tail[j];
    const long d = off[l + 1] + ins[l] + next[l]++;
    for (long b = 0; b < row_bytes; ++b) col[(size_t)(d * row_bytes + b)] = byte_of(n0 + j, b);
  }
  bool same = true;
  for (long r = 0; r < cap && same; ++r)
    for (long b = 0; b < row_bytes; ++b)
      if (col[(size_t)(r * row_bytes + b)] != byte_of(all[r].serial, b)) {
        same = false;
        break;
      }
  CHECK(same);
  // ---- the error returns: nothing may be emitted
  if (n0 - first >= 2 && bounds.back() > 0) {
    long none = 0;
    auto never = [&](const IvfSpreadChunk&) { ++none; };
    CHECK(ivf_spread_plan(n0, first, chunk, bounds.data(), n0 + bounds.back() - 1, row_bytes, (long)bounce.size(),
                          true, nullptr, never) == -1);  // the top destination exceeds the capacity
    std::vector<long> bad(bounds);
    bad.back() = bad[bad.size() - 2] - 1;  // a shift that decreases (or is negative)
    CHECK(ivf_spread_plan(n0, first, chunk, bad.data(), cap + 10, row_bytes, (long)bounce.size(), true, nullptr,
                          never) == -1);
    if (stats[2] > 0)  // a chunk goes through the bounce buffer, and there is none
      CHECK(ivf_spread_plan(n0, first, chunk, bounds.data(), cap, row_bytes, 0, true, nullptr, never) == -1);
    // out of place every chunk is direct and no bounce buffer is needed
    long st2[3];
    CHECK(ivf_spread_plan(n0, first, chunk, bounds.data(), cap, row_bytes, 0, false, st2,
                          [&](const IvfSpreadChunk& c) { CHECK(c.direct == 1); }) == 0);
    CHECK(st2[2] == 0 && st2[1] == stats[1] + stats[2]);
    CHECK(none == 0);
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(12345);
  const int shapes = 400;
  for (int s = 0; s < shapes; ++s) one_shape(rng, s);
  std::printf("%d shapes, %d failures\n", shapes, g_fail);
  return g_fail ? 1 : 0;
}
