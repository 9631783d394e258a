"""The split-pair CRT encryption of a 2049..4096-bit key holder (kernels_crt4.hpp) against the limb-level CPU model of
its schedule (tools/crt4_model.py): the chunked reduction of r, stage A's representative y R mod p_h (< 2 p_h) handed to
d4r_run as the pair (y R, 0), the closing product with the coefficient's pair, the canonical pair and u = A + p_h B.
Each element is checked against pow() (r^(q_h mod (p_h - 1)) mod p_h, r^n coef mod p_h^2, r^n mod n^2); the model
asserts on the way every 64-bit accumulator below 2^64 and the operand bounds the split-pair passes assume (< 2p into
squares, < 4p after a product, R >= 2^24 p_h)."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import crt4_model as M   # noqa: E402


def _keys(golden):
    k = golden["keys"]["4096"]
    rnd = random.Random(4096)
    top = M.prime_below(1 << 2048, rnd)
    return {"golden-4096": (int(k["p"], 16), int(k["q"], 16)),
            "largest-halves": (M.prime_below(top, rnd), top),
            "3072": (M.rand_prime(1536, rnd), M.rand_prime(1536, rnd))}


@pytest.fixture(scope="module")
def keys(golden):
    return _keys(golden)


@pytest.mark.parametrize("name", ["golden-4096", "largest-halves", "3072"])
def test_crt4_model_values_and_bounds(keys, name):
    p, q = sorted(keys[name])
    n = p * q
    ct_words = 2 * ((n.bit_length() + 31) // 32)
    assert M.R >= (1 << 24) * q, "R >= 2^24 p_h"
    mx = M.selfcheck(p, q)
    rs = [0, 1, 5 * p, n * n - 1, (1 << (32 * ct_words)) - 1]
    for r in rs:
        c, m = M.run(p, q, M.words(r, ct_words))
        assert c == pow(r, n, n * n)
        mx = max(mx, m)
    assert mx < 1 << 64


def test_crt4_model_short_r_and_rng_width(keys):
    """one word of r (K = 1), and the 130 words of the device ChaCha20 stream at 4096 bits (K = 3)"""
    p, q = sorted(keys["golden-4096"])
    n = p * q
    for r, nw in ((0xFFFFFFFF, 1), (random.Random(7).getrandbits(32 * 130), 130)):
        c, _ = M.run(p, q, M.words(r, nw))
        assert c == pow(r, n, n * n)


def test_crt4_model_mac_ratio(keys):
    """the chains' lane-MAC count against k_encrypt<8>'s Montgomery chain over the 296 limbs of n^2"""
    p, q = sorted(keys["golden-4096"])
    a, b, e8 = M.mac_count(p, q)
    assert 5.0 < e8 / (a + b) < 6.5
