// Stand-alone check of csrc/fb_cut.hpp (tests/test_fb_cut_cpu.py builds it with the host sanitizers and runs it):
// the planner's rules at every budget threshold, and the digits cut at the plan's offsets reassembling to a_h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fb_cut.hpp"

using namespace fpai;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s: ", #cond);         \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++failures;                              \
    }                                          \
  } while (0)

// The fewest rows K digits of at most cap bits can have while covering kb bits, found without the planner's formula:
// the kb bits dealt out one at a time, each to a narrowest digit (2^w is convex, so evening out never adds rows).
// 0: K digits cannot cover kb.
static uint64_t min_rows(int kb, int K, int cap) {
  if ((long long)K * cap < kb) return 0;
  std::vector<int> w(K, 0);
  for (int bits = 0; bits < kb; ++bits) ++w[bits % K];
  uint64_t r = 0;
  for (int x : w) r += 1ull << x;
  return r;
}

static void check_plan(int kb, int Wmax, uint64_t row_bytes, uint64_t budget, int Kmin) {
  const int Wu = fb_ladder_window(kb, Wmax, row_bytes, budget);
  const FbCut uni = fb_cut_uniform(kb, Wu), c = fb_cut_plan(kb, Wu, Wmax, row_bytes, budget, Kmin);
  const int cap = std::min(Wmax, 24);
  if (!Wu) {   // nothing fits today: nothing fits now
    CHECK(c.K == 0 && c.W == 0 && c.nw == 0, "kb %d Wmax %d budget %llu", kb, Wmax, (unsigned long long)budget);
    return;
  }
  int sum = 0;
  uint64_t rows = 0;
  for (int k = 0; k < c.K; ++k) {
    const int w = fb_cut_width(k, c.W, c.nw);
    CHECK(w >= 1 && w <= 24 && w <= cap, "width %d at %d (kb %d Wmax %d)", w, k, kb, Wmax);
    CHECK(fb_cut_bit(k, c.W, c.nw) == sum, "bit offset at %d", k);
    CHECK(fb_cut_row(k, c.W, c.nw) == rows, "row offset at %d", k);
    CHECK(((uint64_t)k << c.W) + fb_cut_shift(k, c.W, c.nw) == rows, "row shift at %d", k);
    sum += w;
    rows += 1ull << w;
  }
  CHECK(sum >= kb, "widths sum %d < kb %d", sum, kb);
  CHECK(rows == c.rows() && c.bytes(row_bytes) == 2 * rows * row_bytes, "rows");
  CHECK(c.bytes(row_bytes) <= budget, "kb %d Wmax %d: %llu bytes over budget %llu", kb, Wmax,
        (unsigned long long)c.bytes(row_bytes), (unsigned long long)budget);
  CHECK(c.K <= uni.K, "more digits than the uniform cut");
  if (c.K == uni.K) {   // no digit saved: exactly today's plan
    CHECK(c.W == uni.W && c.nw == 0 && c.rows() == ((uint64_t)uni.K << Wu), "kb %d Wmax %d: not the uniform plan", kb, Wmax);
  } else {
    CHECK(c.K >= Kmin, "K %d < Kmin %d", c.K, Kmin);
    CHECK(rows == min_rows(kb, c.K, cap), "kb %d K %d: not the fewest rows", kb, c.K);
  }
  for (int K = Kmin; K < c.K; ++K) {   // K is minimal: no smaller count fits
    const uint64_t r = min_rows(kb, K, cap);
    CHECK(r == 0 || 2 * r * row_bytes > budget, "kb %d Wmax %d budget %llu: K %d fits below K %d", kb, Wmax,
          (unsigned long long)budget, K, c.K);
  }
}

// the digits as k_fb_digits cuts them (a 64-bit window over 32-bit words), put back at their offsets
static void check_reassembly(int kb, const FbCut& c, std::mt19937_64& rng) {
  const int nw32 = (kb + 31) / 32;
  std::vector<uint32_t> a(nw32 + 2, 0), b(nw32 + 2, 0);
  for (int i = 0; i < nw32; ++i) a[i] = (uint32_t)rng();
  if (kb & 31) a[nw32 - 1] &= (1u << (kb & 31)) - 1u;
  for (int k = 0; k < c.K; ++k) {
    const int bit = fb_cut_bit(k, c.W, c.nw), wi = bit >> 5, sh = bit & 31, w = fb_cut_width(k, c.W, c.nw);
    const uint64_t hi = wi + 1 < (int)a.size() ? a[wi + 1] : 0u, lo = wi < (int)a.size() ? a[wi] : 0u;
    const uint32_t d = (uint32_t)((((hi << 32) | lo) >> sh) & ((1u << w) - 1u));
    if (wi < (int)b.size()) b[wi] |= (uint32_t)((uint64_t)d << sh);
    if (wi + 1 < (int)b.size()) b[wi + 1] |= (uint32_t)(((uint64_t)d << sh) >> 32);
  }
  CHECK(a == b, "kb %d cut (%d, %d, %d): the digits do not reassemble to a_h", kb, c.K, c.W, c.nw);
}

int main() {
  std::mt19937_64 rng(20261020);
  long cases = 0;
  for (int kb : {512, 1024, 1023, 1025})
    for (int Wmax : {8, 12, 16, 22, 23, 24}) {
      const uint64_t row_bytes = kb <= 512 ? 224 : 448;
      const int Kmin = kb <= 512 ? 19 : 37, cap = std::min(Wmax, 24);
      // every budget at which a plan can change: each ladder window's tables and each digit count's fewest rows
      std::vector<uint64_t> thr;
      for (int w : {24, 23, 22, 21, 20, 16, 12, 8})
        if (w <= Wmax) thr.push_back(fb_cut_uniform(kb, w).bytes(row_bytes));
      for (int K = 1; K <= (kb + 7) / 8; ++K)
        if (const uint64_t r = min_rows(kb, K, cap)) thr.push_back(2 * r * row_bytes);
      for (uint64_t t : thr)
        for (uint64_t budget : {t - 1, t, t + 1}) {
          check_plan(kb, Wmax, row_bytes, budget, Kmin);
          const int Wu = fb_ladder_window(kb, Wmax, row_bytes, budget);
          const FbCut c = fb_cut_plan(kb, Wu, Wmax, row_bytes, budget, Kmin);
          if (c.K) check_reassembly(kb, c, rng);
          ++cases;
        }
      check_plan(kb, Wmax, row_bytes, ~0ull >> 1, Kmin);   // no cap at all: the asked window, uniform
    }
  // the cases the design rests on (Window trade)
  {
    const uint64_t GB = 1000000000ull;
    FbCut c = fb_cut_plan(1024, 22, 23, 448, 263 * GB, 37);   // a 288-GB device less its reserve, window 23 asked
    CHECK(c.K == 46 && c.W == 22 && c.nw == 12, "headline cut (%d, %d, %d)", c.K, c.W, c.nw);
    CHECK(c.bytes(448) == 2ull * (12 * (1ull << 23) + 34 * (1ull << 22)) * 448, "headline bytes");
    c = fb_cut_plan(1024, 22, 23, 448, 200 * GB, 37);         // without room for it: today's plan
    CHECK(c.K == 47 && c.W == 22 && c.nw == 0, "fallback cut (%d, %d, %d)", c.K, c.W, c.nw);
    c = fb_cut_plan(1024, 22, 22, 448, 263 * GB, 37);         // window 22 asked: no digit may be wider
    CHECK(c.K == 47 && c.W == 22 && c.nw == 0, "asked window (%d, %d, %d)", c.K, c.W, c.nw);
  }
  std::printf("%ld budgets checked, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
