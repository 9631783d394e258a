#!/usr/bin/env python3
"""Edge inputs of the prime search (csrc/kernels_prime.hpp k_mr_w) that are too slow to find at test time, and the
seeded generators the tests share with this tool (tests/test_gpu_prime_edges.py builds its 256- and 512-bit inputs with
them at run time; tests/test_prime_edges_cpu.py recomputes every property this file states).

    python3 tools/make_prime_edges.py          # writes tests/golden/prime_edges.json

Everything is seeded and uses the package's own host functions (flex.crypto.paillier._bigint) only. The file holds,
at 1024 and 2048 bits, hex integers with their claimed properties:

  family A   the smallest prime above 2^(BITS-1) and the largest below 2^BITS; a prime and a composite of a given limb
             shape: a run of ones / of zeros over two whole lanes of the row (28 LW bits each, LW = 3 / 5) and, at
             1024 bits only (m' depends on limb 0 alone), limb 0 equal to 2^28 - 1, limb 0 equal to 1;
  family B   n = d 2^s + 1 for s = 28, 28 LW and BITS / 2, one prime and one composite (without a factor below 2000) each;
  family D   n = (2^t r + 1)(2^(t + 1) r + 1), both factors prime, r odd (so n - 1 = 2^t * odd), t = 1 and t = 3, with
             every strong liar among the bases 0..127 (1024 bits) or 0..47 (2048 bits, where one base costs the host
             25 ms) and the first four from 2^31 on, each with the exit the host's test takes
             (test_gpu_prime._strong_test).

Generation took 56 s on the machine this was written on (one core): 5 s for the 1024-bit records, 51 s for the 2048-bit
ones, most of it the Proth primes and the pairs of prime factors.
"""
import json
import math
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "prime_edges.json")
LIMB = 28                                         # bits per limb (csrc: LB)
LW = {256: 2, 512: 2, 1024: 3, 2048: 5}           # limbs per lane of a row (prime::Geom<K>::LW, K = 10, 19, 37, 74)
LIAR_SCAN = {1024: 128, 2048: 48}                 # the fixture's liars: every one below this ...
LIAR_HIGH = 4                                     # ... and this many from 2^31 on
SHAPES = ("mid_ones", "mid_zeros", "limb0_ones", "limb0_one")


def _bigint():
    for p in (ROOT, os.path.join(ROOT, "ibond-flex_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from flex.crypto.paillier import _bigint
    return _bigint


_PRIMORIAL = None


def no_small_factor(x: int) -> bool:
    """x has no odd prime factor below 2000 (what the device search's sieve lets through)."""
    global _PRIMORIAL
    if _PRIMORIAL is None:
        _PRIMORIAL = math.prod(_bigint()._SMALL_PRIMES)
    return math.gcd(x, _PRIMORIAL) == 1


def is_prime(x: int) -> bool:
    return no_small_factor(x) and _bigint().is_probable_prime(x)


def strong_exit(n: int, a: int):
    """(verdict, exit, squarings done) of the strong test of odd n to base a: test_gpu_prime._strong_test with the depth
    of the squaring tail. The tests take verdicts from _strong_test; this serves preconditions and this tool."""
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    y = pow(a, d, n)
    if y == 1:
        return True, "one", 0
    if y == n - 1:
        return True, "minus_one", 0
    for r in range(1, s):
        y = y * y % n
        if y == n - 1:
            return True, "squared", r
    return False, "never", max(s - 1, 0)


def trailing_zeros(x: int) -> int:
    return (x & -x).bit_length() - 1


def prime_above_half(bits: int) -> int:
    return _bigint().next_prime(1 << (bits - 1))


def prime_below_top(bits: int) -> int:
    c = (1 << bits) - 1
    while not is_prime(c):
        c -= 2
    return c


def shaped(bits: int, shape: str, rng: random.Random) -> int:
    """A random odd `bits`-bit integer of one of SHAPES."""
    lane = LIMB * LW[bits]
    x = rng.getrandbits(bits) | 1 << (bits - 1) | 1
    if shape in ("mid_ones", "mid_zeros"):
        run = ((1 << 2 * lane) - 1) << lane            # lanes 1 and 2 of the row, whole
        x = x | run if shape == "mid_ones" else x & ~run
    elif shape == "limb0_ones":
        x |= (1 << LIMB) - 1
    elif shape == "limb0_one":
        x = x & ~((1 << LIMB) - 1) | 1
    else:
        raise ValueError(shape)
    return x


def has_shape(x: int, bits: int, shape: str) -> bool:
    lane = LIMB * LW[bits]
    mid = x >> lane & ((1 << 2 * lane) - 1)
    return x.bit_length() == bits and {
        "mid_ones": mid == (1 << 2 * lane) - 1, "mid_zeros": mid == 0,
        "limb0_ones": x & ((1 << LIMB) - 1) == (1 << LIMB) - 1, "limb0_one": x & ((1 << LIMB) - 1) == 1}[shape]


def shaped_pair(bits: int, shape: str, seed: int):
    """(a prime, a composite without small factors) of the shape."""
    rng = random.Random(seed)
    prime = comp = None
    while prime is None or comp is None:
        x = shaped(bits, shape, rng)
        if not no_small_factor(x):
            continue
        if _bigint().is_probable_prime(x):
            prime = prime or x
        else:
            comp = comp or x
    return prime, comp


def proth(bits: int, s: int, seed: int, prime: bool):
    """n = d 2^s + 1 of exactly `bits` bits with d odd: a prime, or a composite without a factor below 2000. None where
    there is none: d has bits - s bits, so s = bits - 1 leaves d = 1 and s = bits - 2 leaves d = 3, both composite
    (2^(bits - 1) + 1 is a multiple of 3; 3 * 2^(bits - 2) + 1 has a small factor at every size here)."""
    db = bits - s
    if db <= 2:
        n = ((1 << (db - 1)) | 1) << s | 1
        return None if prime or no_small_factor(n) and _bigint().is_probable_prime(n) else n
    rng = random.Random(seed)
    while True:
        d = rng.getrandbits(db) | 1 << (db - 1) | 1
        n = (d << s) + 1
        if no_small_factor(n) and _bigint().is_probable_prime(n) == prime:
            return n


def liar_semiprime(bits: int, t: int, seed: int, accept=None):
    """(n, p, q): n = p q of exactly `bits` bits with p = 2^t r + 1 and q = 2^(t + 1) r + 1 both prime and r odd, so
    n - 1 = 2^t r (2^(t + 1) r + 3) has exactly t trailing zeros. About a quarter (t = 1) or a sixth (t = 3) of all
    bases are strong liars of such an n. `accept(n)` filters further."""
    rng = random.Random(seed)
    rb = (bits - 2 * t - 1) // 2 + 1
    while True:
        r = rng.getrandbits(rb) | 1 << (rb - 1) | 1
        p, q = (r << t) + 1, (r << (t + 1)) + 1
        n = p * q
        if n.bit_length() != bits or not no_small_factor(n):
            continue
        if pow(2, p - 1, p) != 1 or not is_prime(p) or not is_prime(q):
            continue
        if accept is None or accept(n):
            return n, p, q


def base3_pseudoprime(bits: int, long_gap: bool, seed: int) -> int:
    """A liar_semiprime (t = 1) that is a strong probable prime to base 3, the base of the device search's first pass;
    with long_gap, one whose next prime lies more than 64 above n - 2."""
    def accept(n):
        return strong_exit(n, 3)[0] and (not long_gap or _bigint().next_prime(n - 2) - (n - 2) > 64)
    return liar_semiprime(bits, 1, seed, accept)[0]


def one_without_minus_one(bits: int, w: int, seed: int, bases):
    """(n, [bases that show it]): n = p q of exactly `bits` bits with p = 3 mod 4 prime, q = 5 (p - 1) + 1 prime and
    5 p = -1 mod 2^w, so n - 1 = (p - 1)(5 p + 1) has s >= w + 1 trailing zeros while p - 1 and q - 1 have one each. A base
    that is a fifth power mod q has a^d = +-1 mod p and mod q (d the odd part of n - 1); where the two signs differ,
    a^d is a square root of 1 other than +-1: the tail's first squaring gives 1, n - 1 never comes, and the host answers
    "never" after s - 1 squarings of 1. A test that stops at 1, counts 1 as a pass, or cuts s short errs here. n is
    taken so that at least two of `bases` are such."""
    rng = random.Random(seed)
    lo, hi = math.isqrt((1 << (bits - 1)) // 5) + 1, math.isqrt((1 << bits) // 5)
    c = (-pow(5, -1, 1 << w)) % (1 << w)
    assert c % 4 == 3
    while True:
        p = rng.randrange(lo, hi) >> w << w | c
        q = 5 * (p - 1) + 1
        n = p * q
        if not lo <= p < hi or n.bit_length() != bits or not no_small_factor(n):
            continue
        if pow(2, p - 1, p) != 1 or not is_prime(p) or not is_prime(q):
            continue
        d = (n - 1) >> trailing_zeros(n - 1)
        show = [a for a in bases if pow(a, d, n) not in (1, n - 1) and pow(a, 2 * d, n) == 1]
        if len(show) >= 2:
            return n, show


def liars_of(n: int, below: int, high: int):
    """[(base, exit)] of every strong liar of n among 0..below - 1, then the first `high` from 2^31 on; and the last
    base looked at."""
    out = []
    for a in range(below):
        ok, how, _ = strong_exit(n, a)
        if ok:
            out.append((a, how))
    a, found = 1 << 31, 0
    while found < high:
        ok, how, _ = strong_exit(n, a)
        if ok:
            out.append((a, how))
            found += 1
        a += 1
    return out, a - 1


def main():
    t0 = time.time()
    recs = []
    for bits in (1024, 2048):
        recs.append({"family": "A", "bits": bits, "shape": "above_half", "n": hex(prime_above_half(bits)), "prime": True})
        recs.append({"family": "A", "bits": bits, "shape": "below_top", "n": hex(prime_below_top(bits)), "prime": True})
        for k, shape in enumerate(SHAPES[:4 if bits == 1024 else 2]):
            p, c = shaped_pair(bits, shape, 7000 + bits + k)
            recs.append({"family": "A", "bits": bits, "shape": shape, "n": hex(p), "prime": True})
            recs.append({"family": "A", "bits": bits, "shape": shape, "n": hex(c), "prime": False})
        for s in (28, LIMB * LW[bits], bits // 2):
            for prime in (True, False):
                n = proth(bits, s, 8000 + bits + s, prime)
                recs.append({"family": "B", "bits": bits, "s": s, "n": hex(n), "prime": prime})
        for t in (1, 3):
            n, p, q = liar_semiprime(bits, t, 9000 + bits + t)
            liars, last = liars_of(n, LIAR_SCAN[bits], LIAR_HIGH)
            recs.append({"family": "D", "bits": bits, "t": t, "s": t, "n": hex(n), "p": hex(p), "q": hex(q), "prime": False,
                         "liars": [[a, how] for a, how in liars], "scanned_below": LIAR_SCAN[bits], "scanned_high_to": last})
        print(f"{bits} bits done at {time.time() - t0:.1f} s", file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump({"generator": "tools/make_prime_edges.py", "records": recs}, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(recs)} records in {time.time() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
