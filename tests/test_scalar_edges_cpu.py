"""The case lists of tests/scalar_edges.py against the oracle and the package's per-object host operators, without a GPU:
what the edge scalars encode to (FACTS), which ones raise, what every list holds, and that PaillierEncryptedNumber's
__mul__ and __add__ agree with the oracle on all of them, exceptions included."""
import math

import numpy as np
import pytest

import scalar_edges as SE
from oracle import paillier_oracle as O

DTYPES = [np.int64, np.float64, np.float32]


@pytest.fixture(scope="module")
def key(golden):
    k = golden["keys"]["1024"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def operand(key):
    """One unit mod n^2 as the ciphertext, never modified."""
    rng = np.random.default_rng(1024)
    return int.from_bytes(rng.bytes(264), "little") % key.nsquare


@pytest.mark.parametrize("dt", DTYPES)
def test_lists_as_the_issue_states_them(dt):
    x = SE.scalars(dt)
    assert x.dtype == dt and len(x) == {np.int64: 15, np.float64: 18, np.float32: 11}[dt]
    if dt == np.int64:
        assert set(int(v) for v in x) == {0, 1, -1, 15, -15, 16, -16, 2 ** 60 - 1, 2 ** 60, -2 ** 60, 2 ** 62, -2 ** 62,
                                          2 ** 63 - 1, -(2 ** 63 - 1), -2 ** 63}
    else:
        assert np.isnan(x).sum() == 1 and np.isposinf(x).sum() == 1 and np.isneginf(x).sum() == 1
        assert (np.signbit(x) & (x == 0)).sum() == 1 and (~np.signbit(x) & (x == 0)).sum() == 1
        fin = x[np.isfinite(x)]
        assert np.array_equal(SE.scalars(dt, finite_only=True), fin)
    if dt == np.float64:
        assert SE.BELOW_CUT < SE.CUT and np.nextafter(SE.BELOW_CUT, 1.0) == SE.CUT
        assert set(SE.F64_SUBSET) <= set(v for v in SE.F64 if math.isfinite(v)) and len(SE.F64_SUBSET) == 6
    if dt == np.float32:
        assert float(x[2]) == 2.0 ** -149 and float(np.float32(SE.FLT_MIN)) == 2.0 ** -126
        assert float(np.float32(SE.FLT_MAX)) == (2.0 - 2.0 ** -23) * 2.0 ** 127


@pytest.mark.parametrize("dt", DTYPES)
def test_every_list_holds_the_window_and_sign_classes(key, dt):
    """A negative scalar, a zero, and the longest window walk the dtype can ask for: 16 windows for int64 (|M| of 61 bits
    or more). A float's mantissa |v| 16^e has 50 to 53 bits, 13 or 14 windows, so no float reaches 16: the float64 list
    must hold a 14-window scalar, the float32 list (whose edges all have 50-bit mantissas) a 13-window one. The shortest
    and the longest walk sit in one list, so they share a wave in the one-call runs."""
    enc = [SE.mantissa(SE.py(v, dt), key) for v in SE.scalars(dt, finite_only=True)]
    wins = [SE.windows(M) for M, _ in enc]
    assert any(M < 0 for M, _ in enc) and any(M == 0 for M, _ in enc)
    assert max(wins) == {np.int64: 16, np.float64: 14, np.float32: 13}[dt] and min(wins) == 0
    if dt == np.int64:
        assert {0, 1, 2, 15, 16} <= set(wins)


def test_every_finite_scalar_encodes_and_the_quoted_facts_hold(key):
    for dt in DTYPES:
        for v in SE.scalars(dt, finite_only=True):
            M, e = SE.mantissa(SE.py(v, dt), key)
            assert (M < 0) == (v < 0 and M != 0) and (dt != np.int64 or (M, e) == (int(v), 0))
    for name, (v, dt, sign, bits, e) in SE.FACTS.items():
        assert any(SE.py(u, dt) == SE.py(v, dt) for u in SE.scalars(dt, finite_only=True)), name
        M, ex = SE.mantissa(SE.py(dt(v), dt), key)
        assert ((M > 0) - (M < 0), ex) == (sign, e), name
        if bits is not None:
            assert abs(M).bit_length() == bits, name
    assert SE.mantissa(2 ** 60 - 1, key)[0] == int("f" * 15, 16) and SE.windows(2 ** 60 - 1) == 15
    assert SE.windows(2 ** 60) == SE.windows(SE.INT64_MAX) == SE.windows(SE.INT64_MIN) == 16
    assert SE.mantissa(float(np.nextafter(SE.CUT, 1.0)), key)[1] == 179      # the cut is at 1e-200 itself


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_non_finite_scalars_raise_in_the_oracle(key, operand, dt):
    for v, exc in ((SE.NAN, ValueError), (SE.INF, OverflowError), (-SE.INF, OverflowError)):
        s = SE.py(dt(v), dt)
        assert SE.expect_mul(operand, 3, s, key) is exc
        with pytest.raises(exc):
            O.mul_scalar(operand, 3, s, key)
        for me in SE.add_plain_exps(s, dt, key):
            assert SE.expect_add(operand, me, s, key) is exc, me
            want = SE.EL_ENC_RANGE if math.isnan(v) else SE.EL_FLOAT_OVF
            assert SE.expect_add_status(operand, me, s, key) == (want, None)
        with pytest.raises(exc):
            O.add_scalar(operand, 0, s, key)


def test_factor_one_rule(key, operand):
    """A term whose scalar does not encode is (1, exp + 0) under factor_one and the oracle's exception without it."""
    cs, es = [operand, operand * 3 % key.nsquare], [4, -2]
    x = np.array([[2.0], [SE.NAN]])
    with pytest.raises(ValueError):
        SE.expect_dot(cs, es, 1, 2, x, 1, key)
    with pytest.raises(OverflowError):
        SE.expect_segdot(cs, es, [0, 1], [0, 2], np.array([1.0, -SE.INF]), key)
    c0, e0 = O.mul_scalar(cs[0], 4, 2.0, key)
    assert SE.expect_dot(cs, es, 1, 2, x, 1, key, factor_one=True) == [O.add_k([c0, 1], [e0, -2], key)]
    got = SE.expect_segdot(cs, es, [1, 0], [0, 0, 1, 2], np.array([SE.INF, 1.0]), key, factor_one=True)
    assert got == [(1, SE.INT32_MIN), (1, -2), O.mul_scalar(cs[0], 4, 1.0, key)]


@pytest.mark.parametrize("dt", DTYPES)
def test_host_operators_agree_with_the_oracle(key, operand, dt):
    """PaillierEncryptedNumber.__mul__ and __add__, the path the package takes without a GPU and for every element the
    device flags: the oracle's bits for every edge scalar, and its exception class where it raises. (Ciphertext exponents
    from -60 up: raising one by 16^256 or more is past max_int at 1024 bits, where the reference's __mul__(factor)
    refuses what the oracle's bare pow does not.)"""
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.keypair import PaillierPublicKey
    pk = PaillierPublicKey(key.n)
    for v in SE.scalars(dt):
        s = SE.py(v, dt)
        for e in ((3,) if dt == np.int64 else (-60, 0, 255)):
            enc = PaillierEncryptedNumber(pk, operand, e)
            for op, want in ((lambda: enc * s, SE.expect_mul(operand, e, s, key)),
                             (lambda: enc + s, SE.expect_add(operand, e, s, key))):
                if isinstance(want, type):
                    with pytest.raises(want):
                        op()
                else:
                    got = op()
                    assert (got.ciphertext(False), got.exponent) == want, (v, e)
