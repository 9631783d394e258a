"""The fixed-point codec at its edges, on every decrypt route and encrypt route, against tests/codec_edges.py (whose
lists and expected results test_codec_edges_cpu.py validates without a GPU).

Decode: decode_element (csrc/kernels.hpp: k_decrypt<1>, <2>, <4> and k_dec4_fin) and decode_lane<37>, <74>
(csrc/kernels_dec.hpp: the pair and row decryptions) are two hand-written copies of the one piece of rounding code in the
library. The ciphertext of a plaintext residue x is c = (1 + n x) mod n^2, which decrypts to x exactly without a modular
power; the first eight of a key carry a real r^n. Status, the bits of val (so -0.0 and denormals count), mant and the raw
words are compared with the expectation on the routes "rows", "above" and "group", and the routes with each other.

Encode: encode_float / encode_int / encode_elem (csrc/device_ops.hpp) under PAI_OBF_NONE for the three dtypes and both
exponent modes: status, exponent and c == (1 + n (m mod n)) mod n^2; a subset with explicit r over the encrypt routes;
and every float that encoded decrypts to the oracle's decode of its encoding, to its own bits where that is exact (a
float64 keeps 50 to 53 bits under PAI_EXP_AUTO, a float32 all of its 24)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import codec_edges as CE
from oracle import paillier_oracle as O
from test_gpu_key_sizes import ENC_ROUTES, _Keys, _native, _Routes

pytestmark = pytest.mark.gpu
DEC_KEYS = ("K512", "K1024", "K1034T", "K1036", "K2048", "K2071", "K2072", "K4096")
ENC_KEYS = ("K1024", "K2071", "K4096")
DEC_ROUTES = (("rows", {}), ("above", {"rows_max": 0}), ("group", {"lane_decrypt": False}))


@pytest.fixture(scope="module")
def K(golden):
    return _Keys(golden)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(N, res, cases, want, what):
    """Every output of one decrypt call against the expectations; all failures are named."""
    val, mant, st, raw = res
    vb, raws, bad = _bits(val), N.words_to_ints(raw), []
    for i, (c, w) in enumerate(zip(cases, want)):
        got = (int(st[i]), int(vb[i]), int(mant[i]))
        if raws[i] != c.x:
            bad.append((c.name, "raw words"))
        elif got[0] != w.st:
            bad.append((c.name, f"status {got[0]}, expected {w.st}"))
        elif w.bits is not None and got[1] != w.bits:
            bad.append((c.name, f"val {float(val[i]).hex()}, expected bits {w.bits:#018x}"))
        elif w.mant is not None and got[2] != w.mant:
            bad.append((c.name, f"mant {got[2]}, expected {w.mant}"))
    assert not bad, f"{what}: {len(bad)} of {len(cases)} cases differ, first {bad[:12]}"


@pytest.mark.parametrize("name", DEC_KEYS)
def test_decode_edges(K, name):
    N = _native()
    ctx, key = K.holder(name)
    n, n2 = key.n, key.nsquare
    cases = CE.decode_cases(key)
    want = [CE.expect_decode(c.x, c.e, n, key.max_int) for c in cases]
    assert {w.st for w in want} >= {CE.EL_OK, CE.EL_INT, CE.EL_INT_BIG, CE.EL_OVERFLOW}
    cs = [(1 + n * c.x) % n2 for c in cases]
    for i in range(8):                               # a real obfuscator on the first eight
        cs[i] = cs[i] * K.r_pow_n(key, O.golden_r(n, 4711, i % 2)) % n2
    assert cs[0] == O.raw_encrypt(cases[0].x, key, O.golden_r(n, 4711, 0)) and cs[9] == O.raw_encrypt(cases[9].x, key, 1)
    for i in (0, 1, 9, len(cs) - 1):
        assert O.raw_decrypt(cs[i], key) == cases[i].x
    ct = N.ints_to_words(cs, ctx.ct_words)
    ex = np.array([c.e for c in cases], dtype=np.int64).astype(np.int32)
    assert [int(e) for e in ex] == [c.e for c in cases]
    res = {}
    for route, opts in DEC_ROUTES:
        with _Routes(ctx, **opts):
            res[route] = ctx.decrypt(ct, ex, want_raw=True)
        _check(N, res[route], cases, want, f"{name} {route}")
    for route in ("above", "group"):
        for x, y in zip(res["rows"], res[route]):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), (name, route)


# --------------------------------------------------------------------------- encode
def _encode_runs(key):
    """[(label, values, exp_mode, fexp, [(status, m, e)])] for one key."""
    N = _native()
    runs = []
    for label, x in (("f64", CE.f64_auto_values()), ("f32", CE.f32_values()), ("i64", CE.i64_auto_values())):
        runs.append((f"{label} auto", x, N.PAI_EXP_AUTO, 0, [CE.expect_encode_auto(v, key) for v in x]))
    for fexp in CE.FIXED_EXPS:
        for label, x in (("f64", CE.f64_fixed_values()), ("f32", CE.f32_values()), ("i64", CE.i64_fixed_values(fexp))):
            runs.append((f"{label} fexp={fexp}", x, N.PAI_EXP_FIXED, fexp, [CE.expect_encode_fixed(v, fexp) for v in x]))
    return runs


def _check_encoded(N, key, ct, ex, st, x, want, what):
    got, bad = N.words_to_ints(ct), []
    for i, (ws, m, e) in enumerate(want):
        if int(st[i]) != ws:
            bad.append((repr(x[i]), f"status {int(st[i])}, expected {ws}"))
        elif ws == CE.EL_OK and (int(ex[i]), got[i]) != (e, CE.c0(m, key)):
            bad.append((repr(x[i]), f"exponent {int(ex[i])}, expected {e}" if int(ex[i]) != e else "ciphertext"))
    assert not bad, f"{what}: {len(bad)} of {len(want)} values differ, first {bad[:12]}"


@pytest.mark.parametrize("name", ENC_KEYS)
def test_encode_edges(K, name):
    N = _native()
    ctx, key = K.holder(name)
    n, mx = key.n, key.max_int
    statuses = set()
    for label, x, mode, fexp, want in _encode_runs(key):
        ct, ex, st = ctx.encrypt(x, mode, fexp, obf_mode=N.PAI_OBF_NONE)
        _check_encoded(N, key, ct, ex, st, x, want, f"{name} {label}")
        statuses |= {(label.split()[0], mode, w[0]) for w in want}
        if mode != N.PAI_EXP_AUTO or label.startswith("i64"):
            continue
        # the round trip of every float that encoded: the oracle's decode of the encoding, and x itself where exact
        ok = np.array([w[0] == CE.EL_OK for w in want])
        val, mant, dst, _ = ctx.decrypt(ct[ok], ex[ok])
        vb, xs, ws = _bits(val), x[ok], [w for w in want if w[0] == CE.EL_OK]
        exact = 0
        for i, (_, m, e) in enumerate(ws):
            back = O.decode(m % n, e, n, mx)
            assert int(dst[i]) == (CE.EL_OK if e > 0 else CE.EL_INT if abs(back) < 2 ** 63 else CE.EL_INT_BIG), (label, xs[i])
            try:
                fb = float(back)
            except OverflowError:                    # the largest double encodes to 2^52 16^243 = 2^1024, an int
                assert abs(back) == 1 << 1024 and int(dst[i]) == CE.EL_INT_BIG
                fb = math.inf if back > 0 else -math.inf
            assert int(vb[i]) == CE.f64_bits(fb), f"{name} {label}: {xs[i]!r} decrypts to {float(val[i]).hex()}"
            if Fraction(float(xs[i])) * Fraction(16) ** e == m and m != 0:
                assert int(vb[i]) == CE.f64_bits(float(xs[i])), (label, xs[i])
                exact += 1
        assert exact >= (len(ws) // 4 if label.startswith("f64") else len(ws) - 4), (label, exact)
    for dt in ("f64", "f32", "i64"):                                   # both statuses met in both modes (ints: fixed only)
        assert (dt, N.PAI_EXP_FIXED, CE.EL_OK) in statuses and (dt, N.PAI_EXP_FIXED, CE.EL_ENC_RANGE) in statuses
        assert (dt, N.PAI_EXP_AUTO, CE.EL_OK) in statuses
    # explicit r: 64 of the values over the encrypt routes
    x = np.concatenate([CE.f64_auto_values()[::47][:50], CE.f64_fixed_values()[-14:]])    # (the non-finite ones among them)
    assert x.size == 64
    rs = [O.golden_r(n, 4711, i % 2) for i in range(64)]
    for mode, fexp in ((N.PAI_EXP_AUTO, 0), (N.PAI_EXP_FIXED, -5)):
        want = [CE.expect_encode_auto(v, key) if mode == N.PAI_EXP_AUTO else CE.expect_encode_fixed(v, fexp) for v in x]
        assert sum(w[0] == CE.EL_OK for w in want) >= 40
        for route in ("rows", "above", "public"):
            with _Routes(ctx, **ENC_ROUTES[route]):
                ct, ex, st = ctx.encrypt(x, mode, fexp, obf_mode=N.PAI_OBF_GIVEN, r=rs)
            got = N.words_to_ints(ct)
            for i, (ws, m, e) in enumerate(want):
                assert int(st[i]) == ws, (name, route, mode, x[i])
                if ws == CE.EL_OK:
                    assert (got[i], int(ex[i])) == (CE.c0(m, key) * K.r_pow_n(key, rs[i]) % key.nsquare, e), (name, route, mode, x[i])


# --------------------------------------------------------------------------- the package
def _package_pick(cases):
    """About 40 of the cases: a spread over the lengths and patterns, then every other one of the sign band, the integer
    seam and zero."""
    special = [c for c in cases if c.cls[0] in ("sign-band", "int-seam", "zero")]
    rest = [c for c in cases if c.cls[0] not in ("sign-band", "int-seam", "zero")]
    return rest[::max(1, len(rest) // 24)][:24] + special[::3]


def test_package_decrypt_types_and_errors(K):
    """PaillierDecryptor on single numbers at the 1024-bit key: the Python type and value are oracle.decode's, an
    integer too wide for int64 is the exact big int, and the two OverflowErrors carry their own messages."""
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    key = K.key("K1024")
    n, mx = key.n, key.max_int
    pub = PaillierPublicKey(n)
    pd = PaillierDecryptor(pub, PaillierPrivateKey(pub, key.p, key.q))
    cases = [c for c in CE.decode_cases(key) if abs(c.e) <= 16]
    pick = _package_pick(cases)
    assert 35 <= len(pick) <= 60
    kinds = set()
    for c in pick:
        num = PaillierEncryptedNumber(pub, (1 + n * c.x) % key.nsquare, c.e)
        try:
            want = O.decode(c.x, c.e, n, mx)
        except OverflowError as err:
            with pytest.raises(OverflowError) as got:
                pd.decrypt(num)
            assert str(got.value) == str(err), c.name
            kinds.add(str(err))
            continue
        got = pd.decrypt(num)
        assert type(got) is type(want), f"{c.name}: {type(got).__name__}, expected {type(want).__name__}"
        if isinstance(want, float):
            assert CE.f64_bits(got) == CE.f64_bits(want), c.name
            kinds.add("float")
        else:
            assert got == want, c.name
            kinds.add("int" if abs(want) < 2 ** 63 else "big int")
    assert kinds >= {"float", "int", "big int", "Overflow detected in decode number"}, kinds
    # "int too large to convert to float" needs a mantissa of 1024 bits: the 2048-bit key
    key = K.key("K2048")
    pub = PaillierPublicKey(key.n)
    pd = PaillierDecryptor(pub, PaillierPrivateKey(pub, key.p, key.q))
    for M, e in ((CE.DBL_TOP, 1), (-CE.DBL_TOP, 5), (CE.DBL_TOP - 1, 1)):
        num = PaillierEncryptedNumber(pub, (1 + key.n * (M % key.n)) % key.nsquare, e)
        try:
            want = O.decode(M % key.n, e, key.n, key.max_int)
        except OverflowError as err:
            with pytest.raises(OverflowError) as got:
                pd.decrypt(num)
            assert str(got.value) == str(err) == "int too large to convert to float"
        else:
            assert CE.f64_bits(pd.decrypt(num)) == CE.f64_bits(want) and M == CE.DBL_TOP - 1
