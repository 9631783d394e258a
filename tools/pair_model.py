"""Limb-level model of the p-adic pair arithmetic mod p^2 (bn_pair.hpp), for checking the algebra
and the accumulator bounds on the host before the kernels change. Not test infrastructure for the
product; run directly: python tools/pair_model.py

A number v mod p^2 is held as a pair (A, B), 0 <= A, B < 2p, with v = A + p B (mod p^2). With
R = 2^(28 S) (S limbs of p), the CIOS product A1 A2 = U R - m p (m the q-digits of the reduction), so
  (A1 + p B1)(A2 + p B2) R^-1 = U + p (A1 B2 + A2 B1 - m) R^-1   (mod p^2)
i.e. the Montgomery product mod p^2 (radix R) is (U, REDC_p(A1 B2 + A2 B1 - m)): 5 S^2 MACs at S limbs
instead of 2 (2S)^2 for a Montgomery product over the 2S limbs of p^2.
"""
import random

LB = 28
MASK = (1 << LB) - 1
I64 = 1 << 64


def limbs(x, S):
    return [(x >> (LB * i)) & MASK for i in range(S)]


def val(l):
    return sum(v << (LB * i) for i, v in enumerate(l))


def wrap64(v):
    v &= I64 - 1
    return v - I64 if v >= (1 << 63) else v


def pair_mul(A1, B1, A2, B2, p, S, sqr=False):
    """Lockstep CIOS over j: P1 <- A1 A2 (+ q1 p), P2 <- B1 A2 + A1 B2 - q1 (+ q2 p). As the kernels do
    (bn_pair.hpp red2), q1 is not subtracted: q2 = (P2_J - q1) pinv makes position J equal q1 mod 2^28 and the
    retiring shift drops it, so P2 stays non-negative (unsigned 64-bit accumulators)."""
    pl = limbs(p, S)
    pinv = (-pow(p, -1, 1 << LB)) % (1 << LB)
    P1 = [0] * S
    P2 = [0] * S
    mx1 = mx2 = 0
    for J in range(S):
        a2j, b2j = A2[J], B2[J]
        if sqr:
            P1[(2 * J) % S] += A1[J] * A1[J]
            for i in range(J + 1, S):
                P1[(i + J) % S] += A1[i] * (2 * A1[J])
            for i in range(S):
                P2[(i + J) % S] += A1[i] * (2 * B1[J])
        else:
            for i in range(S):
                P1[(i + J) % S] += A1[i] * a2j
                P2[(i + J) % S] += B1[i] * a2j + A1[i] * b2j
        q1 = ((P1[J] & MASK) * pinv) & MASK
        for i in range(S):
            P1[(i + J) % S] += q1 * pl[i]
        assert P1[J] & MASK == 0
        P1[(J + 1) % S] += P1[J] >> LB
        P1[J] = 0
        q2 = ((((P2[J] & 0xFFFFFFFF) - q1) & 0xFFFFFFFF) * pinv) & MASK
        for i in range(S):
            P2[(i + J) % S] += q2 * pl[i]
        assert P2[J] >= 0 and P2[J] & MASK == q1
        P2[(J + 1) % S] += P2[J] >> LB   # drops q1: the subtraction of m
        P2[J] = 0
        mx1 = max(mx1, max(P1))
        mx2 = max(mx2, max(P2))
    assert mx1 < (1 << 64) and mx2 < (1 << 64), (mx1.bit_length(), mx2.bit_length())

    def norm(P):
        c, r = 0, []
        for v in P:
            v += c
            r.append(v & MASK)
            c = v >> LB
        assert c == 0, c
        return r
    return norm(P1), norm(P2)


def check(pbits, trials=200, seed=1):
    rng = random.Random(seed)
    S = (pbits + 4 + LB - 1) // LB if pbits == 512 else -(-(pbits + 12) // LB)
    S = {512: 19, 1024: 37, 2048: 74}[pbits]
    R = 1 << (LB * S)
    for _ in range(trials):
        p = rng.getrandbits(pbits) | (1 << (pbits - 1)) | 1
        p2 = p * p
        Rinv = pow(R, -1, p2)
        for sqr in (False, True):
            A1, B1 = rng.randrange(2 * p), rng.randrange(2 * p)
            if sqr:
                A2, B2 = A1, B1
            else:
                A2, B2 = rng.randrange(p), rng.randrange(p)
            U, Bn = pair_mul(limbs(A1, S), limbs(B1, S), limbs(A2, S), limbs(B2, S), p, S, sqr)
            U, Bn = val(U), val(Bn)
            assert U < 2 * p and Bn < 2 * p, (U / p, Bn / p)
            want = (A1 + p * B1) * (A2 + p * B2) * Rinv % p2
            assert (U + p * Bn) % p2 == want
        # first product with the unreduced c0 chunk sum as B1 (< 2^10 p)
        A1, B1 = 1, rng.randrange(1 << 10) * p + rng.randrange(p)
        A2, B2 = rng.randrange(p), rng.randrange(p)
        U, Bn = pair_mul(limbs(A1, S), limbs(B1, S), limbs(A2, S), limbs(B2, S), p, S)
        U, Bn = val(U), val(Bn)
        assert U < 2 * p and Bn < 2 * p
        assert (U + p * Bn) % p2 == (A1 + p * B1) * (A2 + p * B2) * Rinv % p2
    print(f"pbits={pbits} S={S}: {trials} x (mul, sqr, c0-first) ok")


# ---- pair groups (bn_pgroup.hpp): TPI lanes x LL limbs, the second row kept non-negative by LMASK - q1
def pgroup_pass(A, B, a2, b2, p, TPI, LL, sqr=False, start2=0):
    """The CIOS of bn_pgroup.hpp (step<TPI, LL, SQR, B2Z>) over the digits (a2[j], b2[j]), len(a2) a multiple of LL:
    lane t owns limbs [LL t, LL t + LL) of A, B and p and LL rotating 64-bit accumulators per row; per digit
      P1 += A a2j, P2 += B a2j + A b2j (sqr: P2 += A (2 b2j)); q1 from lane 0; P2_low += LMASK - q1 (lane 0); q2;
      P1 += q1 p, P2 += q2 p; both rows shift one limb across the group.
    The second row starts at start2 (an integer < 2^(28 S)). Returns (U, Bn, mx): the two rows as integers and an
    upper bound (exact above bit 32) of the largest value any accumulator held before a shift. The accumulators are
    kept exactly as (high, low) halves in numpy uint64, so the model runs S = 152 in milliseconds."""
    import numpy as np
    S = TPI * LL
    assert len(a2) == len(b2) and len(a2) % LL == 0
    M32 = np.uint64(0xFFFFFFFF)
    sh32 = np.uint64(32)
    Av = np.array(A, dtype=np.uint64).reshape(TPI, LL)
    Bv = np.array(B, dtype=np.uint64).reshape(TPI, LL)
    pv = np.array(limbs(p, S), dtype=np.uint64).reshape(TPI, LL)
    pinv = (-pow(p, -1, 1 << LB)) % (1 << LB)
    hi = [np.zeros((TPI, LL), dtype=np.uint64) for _ in range(2)]
    lo = [np.zeros((TPI, LL), dtype=np.uint64), np.array(limbs(start2, S), dtype=np.uint64).reshape(TPI, LL)]
    mx = 0

    def acc(row, prod, s):      # P[(i + s) % LL] += prod[i]; every product is < 2^58
        prod = np.roll(prod, s, axis=1)
        lo[row] += prod & M32
        hi[row] += prod >> sh32

    def low28(row, s):
        return int(lo[row][0, s]) & MASK

    for j, (aj, bj) in enumerate(zip(a2, b2)):
        s = j % LL
        acc(0, Av * np.uint64(aj), s)
        if sqr:
            acc(1, Av * np.uint64(2 * bj), s)
        else:
            acc(1, Bv * np.uint64(aj), s)
            if bj:
                acc(1, Av * np.uint64(bj), s)
        q1 = (low28(0, s) * pinv) & MASK
        lo[1][0, s] += np.uint64(MASK - q1)
        q2 = (low28(1, s) * pinv) & MASK
        acc(0, pv * np.uint64(q1), s)
        acc(1, pv * np.uint64(q2), s)
        for row in (0, 1):
            mx = max(mx, (int((hi[row] + (lo[row] >> sh32)).max()) << 32) | 0xFFFFFFFF)   # value >> 32 is exact
            v = [(int(hi[row][t, s]) << 32) + int(lo[row][t, s]) for t in range(TPI)]
            assert v[0] & MASK == 0
            for t in range(TPI):
                c = v[t] >> LB
                lo[row][t, (s + 1) % LL] += np.uint64(c & 0xFFFFFFFF)
                hi[row][t, (s + 1) % LL] += np.uint64(c >> 32)
                lo[row][t, s] = np.uint64(v[t + 1] & MASK) if t + 1 < TPI else np.uint64(0)
                hi[row][t, s] = np.uint64(0)
    out = []
    for row in (0, 1):
        out.append(sum(((int(hi[row][t, i]) << 32) + int(lo[row][t, i])) << (LB * (t * LL + i))
                       for t in range(TPI) for i in range(LL)))
    return out[0], out[1], mx


def pgroup_mul(A1, B1, A2, B2, p, TPI, LL, sqr=False):
    """pgrp::montmul<TPI, LL, SQR>: (A1 + p B1)(A2 + p B2) R^-1 mod p^2 as a pair, R = 2^(28 TPI LL); the second row
    starts at (1 - R) mod p. Integers in, (U, Bn, mx) out."""
    S = TPI * LL
    R = 1 << (LB * S)
    if sqr:
        A2, B2 = A1, B1
    return pgroup_pass(limbs(A1, S), limbs(B1, S), limbs(A2, S), limbs(B2, S), p, TPI, LL, sqr, (1 - R) % p)


def pe4_pre(r, n, TPI=8, LL=19):
    """k_pe4_pre (kernels_pe4.hpp): r R mod n^2 as a pair from r's 2 S digits: one B-free pass of the constant pair of
    R^3 mod n^2 whose second row starts at (1 - R^2) mod n. r < 2^(28 2 S). Returns (A, B, mx)."""
    S = TPI * LL
    R = 1 << (LB * S)
    r3 = pow(R, 3, n * n)
    cA, cB = r3 % n, r3 // n
    return pgroup_pass(limbs(cA, S), limbs(cB, S), limbs(r, 2 * S), [0] * (2 * S), n, TPI, LL, False, (1 - R * R) % n)


if __name__ == "__main__":
    check(512)
    check(1024)
    check(2048, trials=20)
