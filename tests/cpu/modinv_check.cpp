// csrc/modinv_step.hpp on the host: the 31-step routine, the row plan, the Montgomery coefficient and the round count,
// driven through a plain multi-word outer loop that forms the same unsigned sums as k_modinv (kernels_inv.hpp). For
// every input a = 0 is reached within modinv_rounds(len(m)) rounds, and x * out = 1 (mod m) by schoolbook product and
// remainder here (where b ends above 1, it divides x and m instead). Built with the sanitizers by test_modinv_cpu.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "modinv_step.hpp"

using namespace fpai;
typedef std::vector<uint32_t> Num;   // little-endian words
typedef unsigned __int128 u128;

static uint64_t rng_state = 1;
static uint32_t rnd() { return (uint32_t)((rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull) >> 32); }
static int cmp(const Num& a, const Num& b) {
  for (size_t i = a.size(); i-- > 0;)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
static bool is_small(const Num& a, uint32_t v) { return a[0] == v && std::all_of(a.begin() + 1, a.end(), [](uint32_t w) { return !w; }); }
// a += sign * b (mod 2^(32 n)); b may be shorter
static void add_to(Num& a, const Num& b, int sign) {
  int64_t c = 0;
  for (size_t i = 0; i < a.size(); ++i) { c += (int64_t)a[i] + sign * (int64_t)(i < b.size() ? b[i] : 0); a[i] = (uint32_t)c; c >>= 32; }
}
static int top_word(const Num& a) {
  int j = (int)a.size() - 1;
  while (j > 0 && !a[j]) --j;
  return j;
}

// (cp P + cn ~N + k M' + cn + sub - 2^(32 n) (cn + sub)) / 2^31, M' = m or ~m: words and sign, as the kernel forms them
static bool apply(const Num& P, const Num& N, ModinvRow r, const Num* m, ModinvK mk, Num& out) {
  const size_t n = P.size();
  const uint64_t sub = (m && mk.neg) ? mk.k : 0;
  uint64_t t = r.cn + sub;
  Num S(n + 1);
  for (size_t i = 0; i < n; ++i) {
    t += (uint64_t)r.cp * P[i] + (uint64_t)r.cn * (uint32_t)~N[i] + (m ? (uint64_t)mk.k * (mk.neg ? (uint32_t)~(*m)[i] : (*m)[i]) : 0);
    S[i] = (uint32_t)t;
    t >>= 32;
  }
  const int64_t top = (int64_t)t - (int64_t)r.cn - (int64_t)sub;
  S[n] = (uint32_t)top;
  for (size_t i = 0; i < n; ++i) out[i] = (S[i] >> 31) | (S[i + 1] << 1);
  return top < 0;
}

// b = gcd and v after the fixed rounds; false when a != 0 at the end
static bool invert(const Num& x, const Num& m, Num& b, Num& v) {
  const size_t n = m.size();
  Num a = x, u(n, 0), zero(n, 0), t[4] = {zero, zero, zero, zero};
  b = m;
  v = zero;
  u[0] = 1;
  const uint32_t ninv = modinv_neg_minv31(m[0]);
  const int mj = top_word(m);
  for (int it = modinv_rounds(32 * mj + 32 - __builtin_clz(m[mj])); it > 0; --it) {
    int jt = (int)n - 1;
    while (jt > 1 && (a[jt] | b[jt]) == 0) --jt;
    const int s = 32 - __builtin_clz(a[jt] | b[jt] | 1);
    auto w64 = [&](const Num& z, int hi) { return ((uint64_t)z[hi] << 32) | z[hi - 1]; };
    const ModinvMat M = modinv_steps31(modinv_approx(w64(a, 1), w64(a, jt), jt, s), modinv_approx(w64(b, 1), w64(b, jt), jt, s));
    const int64_t fg[2][2] = {{M.f0, M.g0}, {M.f1, M.g1}};
    for (int row = 0; row < 2; ++row) {
      ModinvRow p = modinv_row_plan(fg[row][0], fg[row][1], false);
      Num &ab = t[row], &uv = t[2 + row];
      if (apply(p.p_is_b ? b : a, p.p_is_b ? a : b, p, nullptr, ModinvK{0, false}, ab)) {
        Num pos = ab;
        add_to(ab = zero, pos, -1);
        p = modinv_row_plan(fg[row][0], fg[row][1], true);
      }
      const Num &P = p.p_is_b ? v : u, &N = p.p_is_b ? u : v;
      const uint32_t t0 = p.cp * P[0] + p.cn * (uint32_t)~N[0] + p.cn;
      if (apply(P, N, p, &m, modinv_row_k(t0, p.cp, ninv), uv)) add_to(uv, m, 1);
    }
    a = t[0]; b = t[1]; u = t[2]; v = t[3];
  }
  return is_small(a, 0);
}

// P mod d == 0 (d != 0): a quotient word from R's top 96 bits over d's top 64 + 1 never overshoots; the loop adds the rest
static bool divides(const Num& d, Num P) {
  const size_t L = top_word(d) + 1;
  const u128 top = L > 1 ? (((u128)d[L - 1] << 32) | d[L - 2]) + 1 : d[0];
  Num R(L + 1, 0), qd(L + 1), ext(d.begin(), d.begin() + L);
  ext.push_back(0);
  for (size_t i = P.size(); i-- > 0;) {
    R.insert(R.begin(), P[i]);
    R.pop_back();                                             // R = R 2^32 + P[i] < d 2^32
    const u128 num = L > 1 ? ((u128)R[L] << 64) | ((u128)R[L - 1] << 32) | R[L - 2] : ((u128)R[1] << 32) | R[0];
    uint64_t c = 0;
    for (size_t j = 0; j <= L; ++j) { c += (uint64_t)(num / top) * ext[j]; qd[j] = (uint32_t)c; c >>= 32; }
    add_to(R, qd, -1);
    while (cmp(R, ext) >= 0) add_to(R, ext, -1);
  }
  return is_small(R, 0);
}

int main() {
  long cases = 0, failures = 0;
  for (int W : {1, 2, 33, 64, 256}) {
    const size_t n = std::max(W, 2);   // the outer loop reads words 0 and 1
    const int K = (W + 63) / 64;
    auto random_num = [&](int words) { Num r(n, 0); for (int i = 0; i < words; ++i) r[i] = rnd(); return r; };
    auto pow2 = [&](int j) { Num r(n, 0); r[j / 32] = 1u << (j % 32); return r; };
    std::vector<Num> mods(4, Num(n, 0));
    mods[0] = random_num(W); mods[0][0] |= 1; mods[0][W - 1] |= 0x80000000u;            // random, top bit set
    std::fill(mods[1].begin(), mods[1].begin() + W, 0xffffffffu); mods[1][0] -= 18;     // 2^(32W) - 19
    mods[2][W - 1] = 0x80000000u; mods[2][0] |= 1;                                      // 2^(32W-1) + 1
    mods[3] = random_num(W - 1); mods[3][0] |= 1; mods[3][W - 1] = 1;                   // top word 1 (W = 1: m = 1)
    for (size_t mi = 0; mi < mods.size(); ++mi) {
      const Num& m = mods[mi];
      std::vector<Num> xs;
      auto both = [&](const Num& v) {   // v and m - v, where 0 < v < m
        if (cmp(v, m) >= 0 || is_small(v, 0)) return;
        xs.push_back(v);
        xs.push_back(m);
        add_to(xs.back(), v, -1);
      };
      Num half = m;                                                                     // (m + 1) / 2 and (m - 1) / 2
      for (size_t i = 0; i < n; ++i) half[i] = (m[i] >> 1) | (i + 1 < n ? m[i + 1] << 31 : 0);
      both(half);
      for (int j : {0, 1, 31, 32, 63, 64, 32 * K - 1, 32 * K + 1})                      // 1, 2, 2^j and m - each
        if (j < 32 * W) both(pow2(j));
      both(random_num(1));                                                              // one word; top word zero
      both(random_num(W - 1));
      Num f0 = pow2(0), f1 = pow2(1);                                                   // Fibonacci neighbours below m
      for (Num f2 = f1;; f0 = f1, f1 = f2) {
        add_to(f2 = f1, f0, 1);
        if (cmp(f2, f1) < 0 || cmp(f2, m) >= 0) break;                                  // wrapped, or past m
      }
      both(f0); both(f1);
      for (int i = 0; i < 40; ++i) { Num r = random_num(W); r[W - 1] %= m[W - 1]; both(r); }
      for (const Num& x : xs) {
        Num b, v, P(2 * n, 0);
        bool ok = invert(x, m, b, v) && cmp(v, m) < 0;
        for (size_t i = 0; i < n; ++i) {                                                // P = x v
          uint64_t c = 0;
          for (size_t j = 0; j < n; ++j) { c += (uint64_t)x[i] * v[j] + P[i + j]; P[i + j] = (uint32_t)c; c >>= 32; }
          P[i + n] = (uint32_t)c;
        }
        add_to(P, pow2(0), -1);
        // b = 1: x v - 1 = 0 (mod m). A random modulus shares factors with some residues: there b divides both
        ok = ok && (is_small(b, 1) ? !is_small(v, 0) && divides(m, P) : !is_small(b, 0) && divides(b, x) && divides(b, m));
        ++cases;
        if (!ok) std::printf("FAIL W=%d modulus %zu residue %ld\n", W, mi, (long)(++failures, &x - &xs[0]));
      }
    }
  }
  std::printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
