"""The obfuscator-pool arithmetic (ibond-flex_amd/csrc/kernels_pool.hpp: k_pool_split, k_pool_join, k_pool_enc's
pool_apply) as tools/pool_model.py restates it limb by limb, against Python integers: rho = a + n b, the row (a 2^84 mod
n, b), and (1 + n M) rho = a + n ((b + M a) mod n) mod n^2 through three Montgomery digit steps. The model asserts the
kernels' accumulator and range bounds (lazy 64-bit accumulators, values below 2 n ahead of the one conditional
subtraction) on the way. Keys at every lane-group size and at the seams between them, the ragged sizes of
tests/test_gpu_ops_sizes.py. CPU only; the kernels are checked through the C ABI by tests/test_gpu_pool.py."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pool_model as PM  # noqa: E402

KEY_BITS = [512, 1035, 1036, 2071, 2072, 3072, 4096]
LANES = {512: 2, 1035: 2, 1036: 4, 2071: 4, 2072: 8, 3072: 8, 4096: 8}
M_EDGES = [0, 1, -1, 2 ** 28 - 1, -(2 ** 28 - 1), 2 ** 28, -(2 ** 28), 2 ** 56 - 1, -(2 ** 56 - 1), 2 ** 63 - 1,
           -(2 ** 63 - 1), -(2 ** 63) + 1]


def _modulus(nbits, rng):
    """An odd n = p q of exactly nbits bits (the identity needs no more of n)."""
    while True:
        p = rng.getrandbits(nbits // 2) | (1 << (nbits // 2 - 1)) | 1
        q = rng.getrandbits(nbits - nbits // 2) | (1 << (nbits - nbits // 2 - 1)) | 1
        if (p * q).bit_length() == nbits:
            return p * q


_KEYS = {}


def _key(nbits):
    if nbits not in _KEYS:
        _KEYS[nbits] = PM.Key(_modulus(nbits, random.Random(nbits)))
    return _KEYS[nbits]


def _want(k, rho, M):
    return (1 + k.n * M) * rho % (k.n * k.n)


@pytest.mark.parametrize("nbits", KEY_BITS)
def test_split_join_and_product_match_python_integers(nbits):
    k = _key(nbits)
    n, n2 = k.n, k.n * k.n
    assert k.tpi == LANES[nbits]
    rng = random.Random(1000 + nbits)
    edges = [1, 2, n - 1, n, n + 1, n2 - n, n2 - 1]
    rhos = edges + [rng.randrange(n2) for _ in range(32)]
    for t, rho in enumerate(rhos):
        row = PM.split(k, rho)
        a, b = rho % n, rho // n
        assert row == ((a << 84) % n, b), f"row of rho #{t}"
        assert PM.join(k, row) == rho, f"join of rho #{t}"
        # every edge rho meets every edge M; the random rows meet three edge values in turn and three random ones
        if t < len(edges):
            Ms = M_EDGES + [rng.randrange(-(2 ** 63) + 1, 2 ** 63) for _ in range(2)]
        else:
            Ms = [M_EDGES[(3 * t + j) % len(M_EDGES)] for j in range(3)] + \
                 [rng.randrange(-(2 ** 63) + 1, 2 ** 63) for _ in range(3)]
        for M in Ms:
            assert PM.apply(k, row, M) == _want(k, rho, M), f"rho #{t}, M = {M}"


@pytest.mark.parametrize("nbits", KEY_BITS)
def test_reduction_edges(nbits):
    """The ends of the three-digit reduction: a = n - 1 under the largest |M|, and |M| a an exact multiple of n (w = 0,
    where a negative M must give t = 0 and not n)."""
    k = _key(nbits)
    n = k.n
    rng = random.Random(2000 + nbits)
    for b in (0, 1, n - 1, rng.randrange(n)):
        rho = (n - 1) + n * b
        row = PM.split(k, rho)
        for M in (2 ** 63 - 1, -(2 ** 63 - 1), -(2 ** 63) + 1):
            assert PM.apply(k, row, M) == _want(k, rho, M)
    # with gcd(M, n) = 1 (every M below the primes of a real key) |M| a is a multiple of n only for a = 0, rho = n b
    for b in (0, 1, n - 1, rng.randrange(n)):
        rho = n * b
        row = PM.split(k, rho)
        assert row == (0, b)
        for M in (1, -1, 2 ** 63 - 1, -(2 ** 63 - 1), rng.randrange(1, 2 ** 63), -rng.randrange(1, 2 ** 63)):
            assert PM.apply(k, row, M) == _want(k, rho, M)


def test_exact_multiple_with_a_factor_of_n():
    """|M| a = j n with a != 0 needs gcd(M, n) > 1: a modulus with a small prime factor, M a multiple of it."""
    rng = random.Random(5)
    for nbits in (512, 1036, 2072):
        f = 1000003
        while True:
            c = rng.getrandbits(nbits - 20) | (1 << (nbits - 21)) | 1
            n = f * c
            if n.bit_length() == nbits:
                break
        k = PM.Key(n)
        n2 = n * n
        for mult in (1, 12345, (2 ** 63 - 1) // f):
            M = f * mult
            a = c * rng.randrange(1, f)                  # M a = (mult * that) n
            assert a < n and (M * a) % n == 0
            for b in (0, n - 1, rng.randrange(n)):
                rho = a + n * b
                row = PM.split(k, rho)
                for s in (M, -M):
                    assert PM.apply(k, row, s) == _want(k, rho, s)


def test_mac_counts():
    """The counts DESIGN.md quotes: (S/2)^2 + 9 S/2 against 4 S^2 + 3 S."""
    c = PM.mac_counts(148)
    assert c["pool_enc"] == 74 * 74 + 9 * 74 and c["c0_obf_mul"] == 4 * 148 * 148 + 3 * 148
    assert c["c0_obf_mul"] / c["pool_enc"] > 14
