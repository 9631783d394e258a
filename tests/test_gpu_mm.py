"""GPU parity of the fused encrypted-by-plain matrix product (kernels_mm.hpp: k_mm_sign, k_mm_tab, k_mm_acc and the
k_add tree over the chunk partials) through the C ABI and the package: against the reference-generated vectors
(tests/golden/make_golden_mul.py), the oracle (mul_scalar / add_k) and the term path of the same library
(set_matmul_fused(False): k_mul + batch inversion + k_add), bit-exact.

The product library keeps calls of fewer than 16 columns, or too small to fill the chip, on the term path (flexpai.hip
mm_take_fused); the small shapes below run on the test build under $FLEXPAI_MM_ALWAYS=1, which sends every call through
the fused kernels (the same object code in both libraries). test_path_option_and_report and test_package_dot run the
product library at a shape inside the fused class."""
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 5, 2), (1, 16, 1), (1, 17, 1), (3, 33, 2), (1, 70, 3)]


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def gmul():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_mul.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _always_fused(monkeypatch):
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")          # read by the test build only, at every call


@pytest.fixture(scope="module")
def ctxs(golden, xlib):
    N = _native()
    out = {}
    for nb in (1024, 2048):
        k = golden["keys"][str(nb)]
        key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
        out[nb] = (N.Context(key.n, 0, key.p, key.q, lib=xlib), key)
    return out


@pytest.fixture(scope="module")
def spread(ctxs):
    """120 oracle ciphertexts at 1024 bits of values spread over 1e-30 .. 1e30 (exponents 34 .. -16, so D > 0 inside
    every chunk), shared by the cases below and never modified."""
    _, key = ctxs[1024]
    rng = np.random.default_rng(120)
    vals = rng.standard_normal(120) * 10.0 ** rng.integers(-30, 31, 120)
    cs, es = [], []
    for i, v in enumerate(vals):
        c, e = O.encrypt_value(float(v), key, O.golden_r(key.n, 120, i))
        cs.append(c)
        es.append(e)
    assert max(es[:16]) - min(es[:16]) >= 20
    return tuple(cs), tuple(es)


def _scalars(K, d, dt, seed):
    rng = np.random.default_rng(seed)
    if dt == np.int64:
        x = rng.integers(-(2 ** 62), 2 ** 62, (K, d), dtype=np.int64)
        x.flat[::4] = 0
        x.flat[1::7] = 2 ** 62
        x.flat[2::7] = -(2 ** 62)
        return x
    if dt == np.float32:
        x = (rng.standard_normal((K, d)) * 100).astype(np.float32)
        x.flat[::5] = 0.0
        x.flat[1::9] = -1.0
        return x
    x = rng.standard_normal((K, d)) * 10.0 ** rng.integers(-20, 20, (K, d))
    x.flat[::5] = 0.0
    x.flat[1::9] = -1.0
    x.flat[3::13] = -0.0
    return x


def _py(v, dt):
    return int(v) if dt == np.int64 else (np.float32(v) if dt == np.float32 else float(v))


def _oracle_dot(cs, es, m, K, x, d, key):
    out = []
    for i in range(m):
        for j in range(d):
            terms = [O.mul_scalar(cs[i * K + k], es[i * K + k], _py(x[k, j], x.dtype.type), key) for k in range(K)]
            out.append(O.add_k([t[0] for t in terms], [t[1] for t in terms], key))
    return out


def _check_vs_oracle(ctx, key, cs, es, m, K, x, d):
    N = _native()
    ct = N.ints_to_words(list(cs), ctx.ct_words)
    ex = np.array(es, dtype=np.int32)
    out, oe = ctx.matmul(ct, ex, m, K, x, d)
    assert ctx.matmul_path == 2
    got = list(zip(N.words_to_ints(out), (int(e) for e in oe)))
    assert got == _oracle_dot(cs, es, m, K, x, d, key)
    return out, oe


def test_path_option_and_report(golden):
    """Fails without the fused path: the options are unknown there."""
    N = _native()
    assert (N.PAI_OPT_MATMUL_FUSED, N.PAI_OPT_MATMUL_PATH) == (16, 17)
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    ctx = N.Context(key.n, 0)                              # the product library
    assert ctx.matmul_fused and ctx.matmul_path == 0
    # 1 x 4096 times 4096 x 64: four times the terms the dispatch asks for at 1024 bits. Random units mod n^2
    rng = np.random.default_rng(16)
    m, K, d = 1, 4096, 64
    ct = rng.integers(0, 2 ** 32, (K, ctx.ct_words), dtype=np.uint32)
    ct[:, -1] = 0                                          # < 2^(32 (W - 1)) < n^2
    ex = rng.integers(12, 15, K).astype(np.int32)
    x = rng.standard_normal((K, d))
    a, ae = ctx.matmul(ct, ex, m, K, x, d)
    assert ctx.matmul_path == 2
    ctx.set_matmul_fused(False)
    assert not ctx.matmul_fused
    b, be = ctx.matmul(ct, ex, m, K, x, d)
    assert ctx.matmul_path == 1
    assert np.array_equal(a, b) and np.array_equal(ae, be)
    ctx.set_matmul_fused(True)
    assert ctx.matmul_fused
    for ms, Ks, ds in ((1, 4096, 1), (1, 64, 16)):         # one column; too few terms to fill the chip
        ctx.matmul(ct[:ms * Ks], ex[:ms * Ks], ms, Ks, x[:Ks, :ds].copy(), ds)
        assert ctx.matmul_path == 1
    assert ctx.lib.pai_ctx_set_option(ctx.handle, N.PAI_OPT_MATMUL_PATH, 1) != 0   # read-only


@pytest.mark.parametrize("nb", [1024, 2048])
def test_reference_golden_on_the_fused_path(ctxs, gmul, nb):
    N = _native()
    ctx, key = ctxs[nb]
    g = gmul["cases"][str(nb)]
    ct = N.ints_to_words([int(h, 16) for h in g["c"]], ctx.ct_words)
    ex = np.array(g["e"], dtype=np.int32)
    feats = np.array([[float.fromhex(v) for v in row] for row in g["features"]])
    K, d = feats.shape
    out, oe = ctx.matmul(ct, ex, 1, K, feats, d)
    assert ctx.matmul_path == 2
    assert [hex(v) for v in N.words_to_ints(out)] == g["dot_c"] and list(oe) == g["dot_e"]


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("m,K,d", SHAPES)
def test_vs_oracle(ctxs, spread, m, K, d, dt):
    """Every output; K around the chunk of 16 (one chunk, one chunk + 1, three chunks, a last chunk of 6), scalars of
    10^-20 .. 10^20, zeros, -0.0, -1.0 and +-2^62 (16 windows) on ciphertext exponents spread over 50 windows."""
    ctx, key = ctxs[1024]
    cs, es = spread
    _check_vs_oracle(ctx, key, cs[:m * K], es[:m * K], m, K, _scalars(K, d, dt, 3 * K + d), d)


def _device_cts(ctx, count, seed):
    """`count` ciphertexts encrypted on the device (explicit small obfuscators: no tables) of values over 1e-30 .. 1e30"""
    N = _native()
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal(count) * 10.0 ** rng.integers(-30, 31, count)
    r = [int(v) for v in rng.integers(2, 2 ** 62, count)]
    ct, ex, st = ctx.encrypt(vals, obf_mode=N.PAI_OBF_GIVEN, r=r)
    assert np.all(st == 0)
    return ct, ex


def _both_paths(ctx, ct, ex, m, K, x, d):
    out, oe = ctx.matmul(ct, ex, m, K, x, d)
    assert ctx.matmul_path == 2
    ctx.set_matmul_fused(False)
    try:
        ref, re_ = ctx.matmul(ct, ex, m, K, x, d)
        assert ctx.matmul_path == 1
    finally:
        ctx.set_matmul_fused(True)
    assert np.array_equal(out, ref) and np.array_equal(oe, re_)
    return out, oe


def test_fused_equals_term_path_2048(ctxs):
    ctx, _ = ctxs[2048]
    m, K, d = 3, 100, 5
    ct, ex = _device_cts(ctx, m * K, 2048)
    for dt in (np.float64, np.int64):
        _both_paths(ctx, ct, ex, m, K, _scalars(K, d, dt, 7), d)


def test_fused_equals_term_path_4096(golden):
    """Arbitrary random units mod n^2 as ciphertexts (the oracle's r^n is too slow at this size), public key only. Both
    paths share k_add<8> and the word packing, so the 6 outputs are also the oracle's."""
    N = _native()
    n = int(golden["keys"]["4096"]["n"], 16)
    ctx = N.Context(n, 0, lib=_native().load_library(_native().XCHECK_LIB_PATH))
    m, K, d = 2, 20, 3
    rng = np.random.default_rng(4096)
    cs = [int.from_bytes(rng.bytes(1024), "little") % (n * n) for _ in range(m * K)]
    ct = N.ints_to_words(cs, ctx.ct_words)
    ex = rng.integers(-12, 30, m * K).astype(np.int32)
    x = _scalars(K, d, np.float64, 11)
    out, oe = _both_paths(ctx, ct, ex, m, K, x, d)
    got = list(zip(N.words_to_ints(out), (int(e) for e in oe)))
    assert got == _oracle_dot(cs, [int(e) for e in ex], m, K, x, d, O.Key(n))


def test_signs(ctxs, spread):
    """All positive (no inversion, no inverse tables), one negative row, every row negative, a column of zeros only."""
    ctx, key = ctxs[1024]
    cs, es = spread
    m, K, d = 2, 19, 3
    rng = np.random.default_rng(19)
    pos = np.abs(rng.standard_normal((K, d))) + 0.5
    one = pos.copy()
    one[17, 1] = -one[17, 1]
    allneg = pos.copy()
    allneg[:, 0] = -allneg[:, 0]
    zcol = -pos
    zcol[:, 1] = 0.0
    zcol[4, 1] = -0.0
    for x in (pos, one, allneg, zcol):
        out, oe = _check_vs_oracle(ctx, key, cs[:m * K], es[:m * K], m, K, x, d)
    got = _native().words_to_ints(out)                 # zcol: value 1 with the largest exponent of its operands
    for i in range(m):
        assert got[i * d + 1] == 1 and oe[i * d + 1] == max(es[i * K:(i + 1) * K])


def test_not_invertible(ctxs, spread):
    """A ciphertext sharing a factor with n: fine with positive scalars and with a negative scalar in another row,
    ZeroDivisionError (the reference's gmpy_math.invert) once its own row holds a negative scalar."""
    N = _native()
    ctx, key = ctxs[1024]
    cs, es = list(spread[0][:5]), list(spread[1][:5])
    cs[2] = key.p * 12345
    ct = N.ints_to_words(cs, ctx.ct_words)
    ex = np.array(es, dtype=np.int32)
    x = np.array([[1.0, 2.0], [0.5, 3.0], [2.0, 7.0], [4.0, 1.0], [5.0, 6.0]])
    for neg_row in (None, 4):
        xs = x.copy()
        if neg_row is not None:
            xs[neg_row, 1] = -xs[neg_row, 1]
        out, oe = ctx.matmul(ct, ex, 1, 5, xs, 2)
        assert ctx.matmul_path == 2
        got = list(zip(N.words_to_ints(out), (int(e) for e in oe)))
        assert got == _oracle_dot(cs, es, 1, 5, xs, 2, key)
    xs = x.copy()
    xs[2, 0] = -2.0
    with pytest.raises(ZeroDivisionError):
        ctx.matmul(ct, ex, 1, 5, xs, 2)


@pytest.mark.parametrize("entries", [16, 40])
def test_blocking_keeps_the_bits(golden, spread, xlib, monkeypatch, entries):
    """The test build with a table budget of 16 ciphertexts (both signs) splits (3, 40, 2) over i and over k (ranges
    of 16, 16, 8); one of 40 splits over i only."""
    N = _native()
    k = golden["keys"]["1024"]
    ctx = N.Context(int(k["n"], 16), 0, lib=xlib)
    cs, es = spread
    m, K, d = 3, 40, 2
    ct = N.ints_to_words(list(cs[:m * K]), ctx.ct_words)
    ex = np.array(es[:m * K], dtype=np.int32)
    x = _scalars(K, d, np.float64, 40)
    monkeypatch.delenv("FLEXPAI_MM_TABLE_BYTES", raising=False)
    want, we = ctx.matmul(ct, ex, m, K, x, d)
    monkeypatch.setenv("FLEXPAI_MM_TABLE_BYTES", str(entries * 2 * 16 * 74 * 4))   # 16 rows of S = 74 limbs, two signs
    got, ge = ctx.matmul(ct, ex, m, K, x, d)
    assert ctx.matmul_path == 2
    assert np.array_equal(got, want) and np.array_equal(ge, we)


def test_package_dot():
    """PaillierArray.dot on the fused path (4096 x 64 features: inside the dispatch's class) and @ with one column (the
    term path) equal numpy's per-object loop (mirrors test_package_operators; the object loop runs two of the 64
    columns)."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    pe, pd = generate_paillier_encryptor_decryptor(1024, seed=5)
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    enc = pe.encrypt(x)
    feats = np.random.default_rng(2).standard_normal((4096, 64))
    plain = np.asarray(enc)
    got = enc.dot(feats)
    n = plain[0].public_key.n
    assert [c.matmul_path for c in _runtime.cached_contexts() if c.n == n] == [2]
    want = plain.dot(feats[:, [0, 63]])
    for g, w in ((got[0], want[0]), (got[63], want[1]), (enc @ feats[:, 5], plain.dot(feats[:, 5]))):
        assert (g.ciphertext(False), g.exponent) == (w.ciphertext(False), w.exponent)
    assert np.allclose(pd.decrypt(got), x.astype(np.float64).dot(feats), rtol=1e-9, atol=1e-9)
