"""The fused matrix product's schedule (ibond-flex_amd/csrc/kernels_mm.hpp) as the big-int model of tools/mm_model.py
-- 4-bit digits of |M|, the shift by D = E - e whole windows, the sign selecting c or c^-1, zero terms, padding, chunks
of KC operands reduced by the add tree -- against the oracle's mul_scalar + add_k on the 1024-bit golden key. CPU only;
the kernels are checked bit-exactly through the C ABI by tests/test_gpu_mm.py."""
import os
import sys

import numpy as np
import pytest

from oracle import paillier_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mm_model as MM   # noqa: E402


@pytest.fixture(scope="module")
def key(golden):
    k = golden["keys"]["1024"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def cts(key):
    """40 ciphertexts of values spread over 1e-30 .. 1e30: exponents from 34 down to -16. Stand-in obfuscators r^n
    (pow(r, n) at 1024 bits for 40 values is the slow part of a CPU test; any unit mod n^2 is a valid ciphertext for
    the arithmetic under test)."""
    rng = np.random.default_rng(40)
    vals = rng.standard_normal(40) * 10.0 ** rng.integers(-30, 31, 40)
    vals[0], vals[1] = 3.0e-30, -7.0e29
    cs, es = [], []
    for i, v in enumerate(vals):
        m, e = O.encode(float(v), key.n, key.max_int)
        cs.append((key.n * m + 1) * pow(O.golden_r(key.n, 40, i), 2, key.nsquare) % key.nsquare)
        es.append(e)
    assert max(es) - min(es) >= 20
    return cs, es


def _want(cs, es, col, key):
    terms = [O.mul_scalar(c, e, s, key) for c, e, s in zip(cs, es, col)]
    return O.add_k([t[0] for t in terms], [t[1] for t in terms], key)


def _col(K, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "f64":
        x = rng.standard_normal(K) * 10.0 ** rng.integers(-20, 20, K)
        x[::5] = 0.0
        x[1::7] = -1.0
        x[2::11] = -0.0
        return [float(v) for v in x]
    if kind == "f32":
        return list((rng.standard_normal(K) * 100).astype(np.float32))
    x = rng.integers(-1000, 1000, K)
    x[::4] = 0
    x[1::6] = 2 ** 62
    x[3::6] = -(2 ** 62)
    return [int(v) for v in x]


@pytest.mark.parametrize("kc", [16, 32])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 33])
def test_fused_schedule_equals_mul_then_add(key, cts, K, kc):
    cs, es = cts[0][:K], cts[1][:K]
    for kind in ("f64", "f32", "i64"):
        col = _col(K, 100 + K, kind)
        stats = {"squarings": 0, "products": 0}
        assert MM.fused_dot(cs, es, col, key.nsquare, kc, stats) == _want(cs, es, col, key), (kind, K, kc)
        assert stats["products"] > 0 or all(MM.encode(s)[0] == 0 for s in col)


def test_int64_extremes_take_16_windows():
    assert MM.windows(2 ** 62) == 16 and MM.encode(-(2 ** 62)) == (-(2 ** 62), 0)
    assert MM.windows((1 << 53) - 1) == 14 and MM.windows(0) == 0


def test_exponent_spread_reaches_20_windows_inside_a_chunk(key, cts):
    cs, es = cts
    spread = [max(es[k0:k0 + 16]) - min(es[k0:k0 + 16]) for k0 in range(0, 32, 16)]
    assert max(spread) >= 20
    col = _col(33, 5, "f64")
    assert MM.fused_dot(cs[:33], es[:33], col, key.nsquare) == _want(cs[:33], es[:33], col, key)


@pytest.mark.parametrize("kc", [16, 32])
def test_all_zero_column_is_one_with_the_largest_exponent(key, cts, kc):
    cs, es = cts[0][:33], cts[1][:33]
    col = [0.0, -0.0, 0] * 11
    got = MM.fused_dot(cs, es, col, key.nsquare, kc)
    assert got == (1, max(es)) and got == _want(cs, es, col, key)


def test_sign_rows_and_no_inverse(key, cts):
    cs, es = list(cts[0][:5]), cts[1][:5]
    assert MM.neg_rows([[1.0, -0.0], [0.0, -2.0], [1e-300, 3]]) == [False, True, False]
    cs[2] = key.p * 12345
    assert MM.fused_dot(cs, es, [1.0, 2.0, 3.0, 4.0, 5.0], key.nsquare)[0] == \
        _want(cs, es, [1.0, 2.0, 3.0, 4.0, 5.0], key)[0]
    assert MM.fused_dot(cs, es, [-1.0, 2.0, 3.0, 4.0, 5.0], key.nsquare) == _want(cs, es, [-1.0, 2.0, 3.0, 4.0, 5.0], key)
    with pytest.raises(ZeroDivisionError):
        MM.fused_dot(cs, es, [1.0, 2.0, -3.0, 4.0, 5.0], key.nsquare)


def test_counts_match_the_documented_model():
    c = MM.counts(m=1, K=4096, d=64, nw=14, neg=1.0, kc=16)
    assert c["fused_chain_per_chunk"] == 52 + 14 * 16 + 1
    assert c["term_per_chunk"] == 16 * (14 + 52 + 13 + 2 + MM.INV_PER_VALUE) + 16
    assert 4.0 < c["ratio_term_over_fused"] < 5.5
    assert 1.5 < MM.counts(d=1, neg=0.5)["ratio_term_over_fused"] < 3.0
