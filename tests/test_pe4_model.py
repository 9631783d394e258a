"""The pair-group arithmetic of the 4096-bit public-key encryption (ibond-flex_amd/csrc/kernels_pe4.hpp on
bn_pgroup.hpp at TPI = 8, LL = 19, S = 152 limbs of n): a limb-level model of the kernels' CIOS schedule
(tools/pair_model.py pgroup_pass: per-lane rotating accumulators, the second row kept non-negative by LMASK - q1 and
its start constant) checked against plain modular arithmetic, with the bounds the kernels rely on: outputs < 2n and
every 64-bit accumulator below 2^64 at worst-case operands. CPU only; the kernels themselves are checked bit-exactly
through the C ABI by tests/test_gpu_pe4.py."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pair_model as PM  # noqa: E402

TPI, LL = 8, 19
S = TPI * LL
R = 1 << (PM.LB * S)


@pytest.fixture(scope="module")
def modulus():
    """A 4096-bit odd composite: the product of two odd 2048-bit numbers with their top two bits set."""
    rng = random.Random(4096)
    f = [rng.getrandbits(2048) | (3 << 2046) | 1 for _ in range(2)]
    n = f[0] * f[1]
    assert n.bit_length() == 4096 and n & 1 and R >= (1 << 24) * n
    return n


def test_pair_group_product_and_square_at_s152(modulus):
    n = modulus
    n2 = n * n
    Rinv = pow(R, -1, n2)
    rng = random.Random(152)
    cases = [(rng.randrange(2 * n), rng.randrange(2 * n), rng.randrange(2 * n), rng.randrange(2 * n)) for _ in range(40)]
    cases.append((2 * n - 1, 2 * n - 1, n - 1, n - 1))                # the bound's worst case
    for A1, B1, A2, B2 in cases:
        U, Bn, mx = PM.pgroup_mul(A1, B1, A2, B2, n, TPI, LL)
        assert U < 2 * n and Bn < 2 * n
        assert mx < 1 << 64, mx.bit_length()
        assert (U + n * Bn) % n2 == (A1 + n * B1) * (A2 + n * B2) * Rinv % n2
        U, Bn, mx = PM.pgroup_mul(A1, B1, None, None, n, TPI, LL, sqr=True)
        assert U < 2 * n and Bn < 2 * n
        assert mx < 1 << 64, mx.bit_length()
        assert (U + n * Bn) % n2 == pow(A1 + n * B1, 2, n2) * Rinv % n2


def test_pre_stage_puts_r_into_montgomery_form(modulus):
    """k_pe4_pre: the 304-digit B-free pass of the pair of R^3 mod n^2 from (1 - R^2) mod n yields r R mod n^2 as a
    pair that the chain's products accept (components <= 2n: R >= 2^24 n leaves that slack)."""
    n = modulus
    n2 = n * n
    rng = random.Random(304)
    rs = [0, 1, n, n2 - 1, (1 << 8192) - 1] + [rng.getrandbits(8192) for _ in range(20)]
    for r in rs:
        A, B, mx = PM.pe4_pre(r, n, TPI, LL)
        assert A <= 2 * n and B <= 2 * n
        assert mx < 1 << 64, mx.bit_length()
        assert (A + n * B) % n2 == r * R % n2
