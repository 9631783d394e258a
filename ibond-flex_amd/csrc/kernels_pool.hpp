// Pooled obfuscators (include/flexpai.h, "Obfuscator pool"): rho = r^n mod n^2 is drawn ahead of time into a
// ring of the context, and the online step of an encryption is (1 + n M) rho mod n^2 alone. With rho = a + n b, a, b < n,
//
//     (1 + n M) rho  =  a + n ((b + M a) mod n)   (mod n^2)
//
// so the product needs M a mod n (M is the encoder's int64: three 28-bit limbs), one addition mod n and ONE schoolbook
// product n t' over the limbs of n: (S/2)^2 multiply-accumulates against the 4 S^2 of make_c0 + k_obf_mul.
//
// The product runs by rows, like the a B[j] half of the CIOS loop (pool_prod_step): n's limbs stay in registers, t' is read
// digit by digit from the group's LDS slot as a broadcast, and after each digit the accumulators move down one limb; the
// limb that leaves at the bottom is final and replaces the digit just consumed in the slot. After S/2 digits the slot
// holds the low half of c and the accumulators the high half. One LDS read per L multiply-accumulates; the first build
// summed by columns with both operands in LDS (two reads per multiply-accumulate in a loop that does not unroll) and ran
// at 1.8x the composed path where this one was built to do better.
//
// Ring row (internal; pai_pool_put and the tests speak plain rho): 2 PW words, PW = ceil(key bits / 32) -- the W words of a
// ciphertext for every key whose size is a multiple of 32 bits. Words [0, PW) hold a' = a 2^84 mod n, words [PW, 2 PW) hold
// b. a' is a pre-scaled: |M| a mod n is then three Montgomery digit steps a' |M| 2^-84, and a itself comes back from three
// reduction steps over a' alone. Both stay below 2 n and take one cond_sub each.
//
//   k_pool_split<TPI>  rho (W words) -> ring row, once per entry, off the critical path. u = rho R^-1 mod n by S reduction
//                      steps (R = 2^(28 S)), a = u (R^2 mod n) R^-1, a' = u (R^2 2^84 mod n) R^-1, b = (rho - a) / n exactly
//                      by Hensel digits (the CIOS loop over 2^(28 S) - n that collects its quotient digits, as k_decrypt's
//                      L function does).
//   k_pool_enc<TPI>    the hot path, one element per group of TPI lanes like k_obf_mul: fused encode, pool_apply, emit_words.
//   k_pool_join<TPI>   ring row -> plain rho words (pool_apply with M = 0): pai_obfuscate's pooled multiplier and the
//                      composed encryption of PAI_OPT_POOL_FUSED = 0.
//
// Every value mod n is a zero-padded S-limb operand of the whole group (n's limbs above S/2 are zero), so the group
// primitives of bn_group.hpp apply unchanged at every TPI and nothing new crosses a 16-lane DPP row: the digit broadcast
// is bcast0<TPI>, the one-limb shift dpp_from_next inside a group, whose top lane receives the next group's reduced (zero)
// low limb or the row's bound_ctrl zero. The lanes of the upper half hold zeros of n and idle through the digit steps
// and the product (their accumulators only pass limbs down).
//
// Rows are addressed as (head + i) % capacity: one launch serves a take or a fill that wraps.
#pragma once
#include "kernels.hpp"

namespace fpai {

struct PoolRing {
  uint32_t* rows;          // [cap][row_words]
  long long cap, first;    // entries; the ring index of the call's element 0
  int row_words, pt_words; // 2 PW, PW
};

struct PoolSplitParams {
  const uint32_t* rho;     // [n][ct_words] plain rho words, each < n^2
  PoolRing ring;
  long long n;
  const uint32_t* nl;      // n limbs (S, zero padded)
  const uint32_t* nneg;    // 2^(28 S) - n
  const uint32_t* R2n;     // R^2 mod n
  const uint32_t* R2n84;   // R^2 2^84 mod n
  uint32_t nprime, dprime; // -n^-1, -(2^(28 S) - n)^-1 = n^-1 mod 2^28
  int ct_words;
};

struct PoolEncParams {
  EncPlain src;            // k_pool_join: unused
  PoolRing ring;
  EncOut dst;              // k_pool_join: ct only
  long long n;
  const uint32_t* nl;      // n limbs (S, zero padded)
  uint32_t nprime;
};

// One Montgomery digit step over n: P <- (P + a d + q n) / 2^28 with q = -P_0 n^-1 mod 2^28. Not rotating (three steps, not
// a multiple of L): the accumulators move down one place instead.
template <int TPI, bool MUL>
__device__ __forceinline__ void pool_digit(uint64_t (&P)[L], const uint32_t (&a)[L], uint32_t d, const uint32_t (&m)[L],
                                           uint32_t nprime) {
  if constexpr (MUL) {
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] += (uint64_t)a[i] * d;
  }
  const uint32_t q = bcast0<TPI>(((uint32_t)P[0] * nprime) & LMASK);
#pragma unroll
  for (int i = 0; i < L; ++i) P[i] += (uint64_t)q * m[i];
  const uint64_t v0 = P[0];
#pragma unroll
  for (int i = 0; i + 1 < L; ++i) P[i] = P[i + 1];
  P[0] += v0 >> LB;
  P[L - 1] = (uint64_t)dpp_from_next((uint32_t)v0 & LMASK);
}

// One row of c = a + n t': P += n t'_j, then the accumulators move down one limb (rotating indices, as in cios_step). The
// limb leaving the group's lowest lane is limb j of c, final since every product that reaches it is in: it is stored over
// the digit just read. The group's top lane takes 0, not the next group's limb. An accumulator lives L rows and takes one
// product below 2^56 per row and one carry: under 2^62.
template <int TPI, int S_>
__device__ __forceinline__ void pool_prod_step(uint64_t (&P)[L], const uint32_t (&m)[L], uint32_t* Bo, uint32_t& bcur,
                                               bool lowest, bool top) {
  const uint32_t bj = bcur;
  if constexpr (S_ + 1 < L) bcur = Bo[S_ + 1];
#pragma unroll
  for (int i = 0; i < L; ++i) P[(i + S_) % L] += (uint64_t)m[i] * bj;
  const uint64_t v0 = P[S_];
  P[(S_ + 1) % L] += v0 >> LB;
  const uint32_t lo = (uint32_t)v0 & LMASK;
  if (lowest) Bo[S_] = lo;
  const uint32_t in = dpp_from_next(lo);
  P[S_] = top ? 0u : in;
#pragma unroll
  for (int i = 0; i < L; ++i) asm volatile("" : "+v"(P[i]));
  __builtin_amdgcn_sched_barrier(0);
}
template <int TPI, int... Ss>
__device__ __forceinline__ void pool_prod_outer(uint64_t (&P)[L], const uint32_t (&m)[L], uint32_t* Bo, bool lowest, bool top,
                                                std::integer_sequence<int, Ss...>) {
  uint32_t bcur = Bo[0];
  (pool_prod_step<TPI, Ss>(P, m, Bo, bcur, lowest, top), ...);
}

// This lane's L limbs of the nw-word integer at slot[off ..), zero above it
__device__ __forceinline__ void pool_cut(const uint32_t* slot, int off, int nw, uint32_t (&x)[L], int tig) {
  int t = tig;
  asm volatile("" : "+v"(t));
  const int base = t * L * LB;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int bit = base + i * LB, j = bit >> 5;
    const uint32_t lo = j < nw ? slot[off + j] : 0u, hi = j + 1 < nw ? slot[off + j + 1] : 0u;
    x[i] = __builtin_amdgcn_alignbit(hi, lo, bit & 31) & LMASK;
  }
}

// c = (1 + n M) rho mod n^2 from rho's ring row: a + n ((b + M a) mod n), canonical (at most n^2 - 1: no final
// subtraction), left as S limbs in the group's slot (pool_emit writes the words). m: n's limbs in registers. Restated limb
// by limb in tools/pool_model.py.
template <int TPI>
__device__ __forceinline__ void pool_apply(uint32_t* slot, const uint32_t* __restrict__ row, const PoolRing& rg, int64_t M,
                                           const uint32_t (&m)[L], uint32_t nprime, int lane, int tig) {
  wave_lds_fence();                                   // earlier readers of the slot are done
  if ((rg.row_words & 3) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(row);
    uint4* d4 = reinterpret_cast<uint4*>(slot);
    for (int q = tig; q < rg.row_words / 4; q += TPI) d4[q] = s4[q];
  } else {
    for (int j = tig; j < rg.row_words; j += TPI) slot[j] = row[j];
  }
  wave_lds_fence();
  // the row's words stay in the slot until t' replaces them: a' and b are cut out where they are needed, so that at
  // most five L-limb values and one set of accumulators are live at a time

  const bool neg = M < 0;
  const uint64_t mag = neg ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
  const uint32_t M0 = (uint32_t)mag & LMASK, M1 = (uint32_t)(mag >> LB) & LMASK, M2 = (uint32_t)(mag >> (2 * LB));
  uint32_t w[L];
  uint64_t P[L];
  // w = |M| a mod n = a' |M| 2^-84 mod n: below (n 2^84 + 2^84 n) / 2^84 = 2 n before the subtraction
  {
    uint32_t ap[L];
    pool_cut(slot, 0, rg.pt_words, ap, tig);
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = 0;
    pool_digit<TPI, true>(P, ap, M0, m, nprime);
    pool_digit<TPI, true>(P, ap, M1, m, nprime);
    pool_digit<TPI, true>(P, ap, M2, m, nprime);
    normalize<TPI>(P, w, lane, tig);
    cond_sub<TPI>(w, m, lane, tig);
  }
  // t' = (b + M a) mod n: b + w less n where that reaches n, or b - w plus n where it borrows (the wrapped difference
  // plus n carries out of the group's top limb; normalize drops that carry). Both are formed: the sign differs per group
  uint32_t tp[L];
  {
    uint32_t b[L], d[L];
    pool_cut(slot, rg.pt_words, rg.pt_words, b, tig);
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = (uint64_t)b[i] + w[i];
    normalize<TPI>(P, tp, lane, tig);
    cond_sub<TPI>(tp, m, lane, tig);
    const bool borrow = sub_limbs<TPI>(b, w, d, lane, tig);
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = (uint64_t)d[i] + (borrow ? m[i] : 0u);
    normalize<TPI>(P, d, lane, tig);
#pragma unroll
    for (int i = 0; i < L; ++i) tp[i] = neg ? d[i] : tp[i];
  }
  // a = a' 2^-84 mod n
  uint32_t a[L];
  {
    uint32_t ap[L];
    pool_cut(slot, 0, rg.pt_words, ap, tig);
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = ap[i];
    pool_digit<TPI, false>(P, ap, 0u, m, nprime);
    pool_digit<TPI, false>(P, ap, 0u, m, nprime);
    pool_digit<TPI, false>(P, ap, 0u, m, nprime);
    normalize<TPI>(P, a, lane, tig);
    cond_sub<TPI>(a, m, lane, tig);
  }
  // c = a + n t' by rows over the S / 2 digits of t' (n and t' have no more): the low half of c lands in the slot, digit
  // by digit; the high half is what the accumulators hold at the end, on the lanes of the lower half
  write_limbs_lds<TPI>(slot, tp, tig);
#pragma unroll
  for (int i = 0; i < L; ++i) P[i] = a[i];
  for (int o = 0; o < TPI / 2; ++o)
    pool_prod_outer<TPI>(P, m, slot + o * L, tig == 0, tig == TPI - 1, std::make_integer_sequence<int, L>{});
  normalize<TPI>(P, a, lane, tig);
  wave_lds_fence();
  if (tig < TPI / 2) {
#pragma unroll
    for (int i = 0; i < L; ++i) slot[(TPI / 2 + tig) * L + i] = a[i];
  }
  wave_lds_fence();
}

// The words of the S canonical limbs pool_apply left in the slot (emit_words without its copy into the slot)
template <int TPI>
__device__ __forceinline__ void pool_emit(uint32_t* slot, uint32_t* __restrict__ out, int nwords, bool valid, int tig) {
  if (valid) {
    for (int j = tig; j < nwords; j += TPI) out[j] = limbs_word(slot, TPI * L, j);
  }
  wave_lds_fence();
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pool_enc(PoolEncParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.nl, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    int64_t M = 0;
    int e = 0;
    const int st = encode_elem(p.src.x, p.src.dtype, p.src.exp_mode, p.src.fexp, t, M, e);
    const uint32_t* row = p.ring.rows + ((p.ring.first + t) % p.ring.cap) * p.ring.row_words;
    pool_apply<TPI>(slot, row, p.ring, M, m, p.nprime, lane, tig);
    pool_emit<TPI>(slot, p.dst.ct + t * p.dst.ct_words, p.dst.ct_words, valid, tig);
    if (valid && tig == 0) {
      p.dst.exp[t] = e;
      if (p.dst.status) p.dst.status[t] = st;
    }
  }
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pool_join(PoolEncParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.nl, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    const uint32_t* row = p.ring.rows + ((p.ring.first + t) % p.ring.cap) * p.ring.row_words;
    pool_apply<TPI>(slot, row, p.ring, 0, m, p.nprime, lane, tig);
    pool_emit<TPI>(slot, p.dst.ct + t * p.dst.ct_words, p.dst.ct_words, valid, tig);
  }
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pool_split(PoolSplitParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.nl, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    uint32_t x[L], u[L], r[L];
    stage_words_to_limbs<TPI>(slot, p.rho + t * p.ct_words, p.ct_words, x, tig);
    // u = rho R^-1 mod n: rho < n^2 < n R, so u < 2 n
    {
      uint64_t P[L];
#pragma unroll
      for (int i = 0; i < L; ++i) P[i] = x[i];
      uint32_t dummy[L];
      cios<TPI, false, false>(P, dummy, nullptr, TPI, m, p.nprime, tig, dummy);
      normalize<TPI>(P, u, lane, tig);
    }
    uint32_t* row = p.ring.rows + ((p.ring.first + t) % p.ring.cap) * p.ring.row_words;
    // a' = rho 2^84 mod n
    copy_g_to_lds<TPI>(slot, p.R2n84, tig);
    montmul<TPI>(r, u, slot, TPI, m, p.nprime, lane, tig);
    cond_sub<TPI>(r, m, lane, tig);
    emit_words<TPI>(slot, r, row, p.ring.pt_words, valid, tig);
    // a = rho mod n, b = (rho - a) / n: the digits q_j = T_0 n^-1 of T <- (T + q_j (R - n)) / 2^28
    copy_g_to_lds<TPI>(slot, p.R2n, tig);
    montmul<TPI>(r, u, slot, TPI, m, p.nprime, lane, tig);
    cond_sub<TPI>(r, m, lane, tig);
    (void)sub_limbs<TPI>(x, r, u, lane, tig);          // rho - a >= 0
    {
      uint64_t P[L];
      uint32_t nn[L], dummy[L];
#pragma unroll
      for (int i = 0; i < L; ++i) {
        P[i] = u[i];
        r[i] = 0;
      }
      load_limbs_g<TPI>(p.nneg, nn, tig);
      cios<TPI, false, true>(P, dummy, nullptr, TPI, nn, p.dprime, tig, r);
    }
    emit_words<TPI>(slot, r, row + p.ring.pt_words, p.ring.pt_words, valid, tig);
  }
}

}  // namespace fpai
