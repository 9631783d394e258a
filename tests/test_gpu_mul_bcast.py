"""GPU parity of the broadcast multiply (pai_mul_bcast[_dev]; kernels_mulb.hpp: k_mulb_plan, k_mulb_tab, k_mulb_acc)
through the C ABI and the package: every output against the oracle's mul_scalar on Python integers, the comb
(PAI_OPT_MUL_BCAST = 2) against the term path (0) of the same library, bit-exact."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f64": np.float64, "f32": np.float32, "i64": np.int64}
I64_MIN = np.iinfo(np.int64).min


def _native():
    from flex.crypto.paillier import _native
    return _native


@functools.lru_cache(maxsize=None)
def _key(nb):
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        k = json.load(f)["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def ctxs(xlib):
    return {nb: _native().Context(_key(nb).n, 0, lib=xlib) for nb in (1024, 2048, 4096)}


@pytest.fixture(autouse=True)
def _default_budget(monkeypatch):
    monkeypatch.delenv("FLEXPAI_MM_TABLE_BYTES", raising=False)
    monkeypatch.delenv("FLEXPAI_MULB_SLICE_BYTES", raising=False)


@functools.lru_cache(maxsize=None)
def _cts(nb, N, seed=0):
    """N random residues mod n^2 (units, but for a chance of 2^-500) with exponents mixed in [-40, 40]."""
    rng = np.random.default_rng(1000 * seed + N)
    nsq = _key(nb).nsquare
    return (tuple(int.from_bytes(rng.bytes(nb // 4 + 8), "little") % nsq for _ in range(N)),
            tuple(int(e) for e in rng.integers(-40, 41, N)))


def _scalars(dt, N, F):
    """Mixed signs and magnitudes with the encoder's edges strewn in, and (N > 1) a last row of zeros."""
    rng = np.random.default_rng(N * 1000 + F)
    if dt == np.int64:
        x = rng.integers(-(2 ** 62), 2 ** 62, (N, F), dtype=np.int64)
        edges = [0, -1, 15, 2 ** 62, -(2 ** 62), I64_MIN, np.iinfo(np.int64).max]
    else:
        x = (rng.standard_normal((N, F)) * 10.0 ** rng.integers(-6, 7, (N, F))).astype(dt)
        edges = [0.0, -0.0, np.nextafter(dt(0), dt(1)), 2.0 ** 62, -(2.0 ** 62), -1.0, 1e-30]      # the third: a denormal
    for k, v in enumerate(edges):
        x.flat[k + 1::11] = v                               # element 0 stays random: (1, 1) multiplies by a non-zero scalar
    if N > 1:
        x[N - 1] = 0
    return x


def _py(v):
    return int(v) if isinstance(v, np.int64) else (v if isinstance(v, np.float32) else float(v))


def _oracle(nb, cs, es, x):
    key = _key(nb)
    return [O.mul_scalar(cs[i], es[i], _py(x[i, j]), key) for i in range(x.shape[0]) for j in range(x.shape[1])]


def _run(ctx, path, cs, es, x):
    N = _native()
    ctx.mul_bcast_mode = path
    out, oe, st = ctx.mul_bcast(N.ints_to_words(list(cs), ctx.ct_words), np.array(es, dtype=np.int32), x)
    assert ctx.mul_bcast_path == (2 if path == 2 else 1)
    return out, oe, st


def _pairs(out, oe):
    return list(zip(_native().words_to_ints(out), (int(e) for e in oe)))


@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("shape", [(1, 1), (3, 17), (5, 64), (2, 130)])      # 17 and 130 leave tail column tiles
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_bit_exact_against_the_oracle(ctxs, dt, shape, path):
    cs, es = _cts(1024, shape[0])
    x = _scalars(DTYPES[dt], *shape)
    out, oe, st = _run(ctxs[1024], path, cs, es, x)
    assert not st.any()
    assert _pairs(out, oe) == _oracle(1024, cs, es, x)
    if path == 2:
        for got, want in zip((out, oe, st), _run(ctxs[1024], 0, cs, es, x)):
            assert np.array_equal(got, want)


def test_rows_with_different_top_windows(ctxs):
    """One launch: digits in window 0 only, full 64-bit magnitudes (INT64_MIN among them), an all-negative row."""
    rng = np.random.default_rng(3)
    x = np.stack([rng.integers(0, 16, 40), rng.integers(2 ** 62, 2 ** 63 - 1, 40) * rng.choice([-1, 1], 40),
                  -rng.integers(1, 2 ** 20, 40)]).astype(np.int64)
    x[1, 7] = I64_MIN
    cs, es = _cts(1024, 3)
    out, oe, st = _run(ctxs[1024], 2, cs, es, x)
    assert not st.any() and _pairs(out, oe) == _oracle(1024, cs, es, x)


@pytest.mark.parametrize("nb", [2048, 4096])
def test_wider_keys(ctxs, nb):
    cs, es = _cts(nb, 3)
    x = _scalars(np.float64, 3, 33)
    out, oe, st = _run(ctxs[nb], 2, cs, es, x)
    for got, want in zip((out, oe, st), _run(ctxs[nb], 0, cs, es, x)):
        assert np.array_equal(got, want)
    got, key = _pairs(out, oe), _key(nb)
    for t in (0, 3, 32, 33, 50):
        assert got[t] == O.mul_scalar(cs[t // 33], es[t // 33], float(x.flat[t]), key)


def test_table_blocks_keep_the_bits(ctxs, monkeypatch):
    """A table budget of 16 combs (the test build reads it at every call): 40 rows take three blocks."""
    cs, es = _cts(1024, 40)
    x = _scalars(np.float64, 40, 9)
    want = _run(ctxs[1024], 2, cs, es, x)
    monkeypatch.setenv("FLEXPAI_MM_TABLE_BYTES", str(16 * 16 * 16 * 74 * 4))       # 16 windows of 16 rows of S = 74 limbs
    for got, w in zip(_run(ctxs[1024], 2, cs, es, x), want):
        assert np.array_equal(got, w)
    assert _pairs(want[0], want[1])[::37] == _oracle(1024, cs, es, x)[::37]


def test_host_slices_keep_the_bits(ctxs, monkeypatch):
    """A slice budget of one row of output (the test build reads it at every call): five rows move in five slices with
    the same bits. That the slices are taken shows where a ciphertext without inverse ends such a call: the rows of
    the slices before its own have been written, as the header says, its own and the later ones have not."""
    N, ctx = _native(), ctxs[1024]
    cs, es = _cts(1024, 5)
    x = _scalars(np.float64, 5, 9)
    want = _run(ctx, 2, cs, es, x)
    monkeypatch.setenv("FLEXPAI_MULB_SLICE_BYTES", str(9 * ctx.ct_words * 4))
    for path in (0, 2):
        for got, w in zip(_run(ctx, path, cs, es, x), want):
            assert np.array_equal(got, w)
    cs = list(cs)
    cs[3] = _key(1024).p
    x[3, 2] = -1.0
    ct, ex = N.ints_to_words(cs, ctx.ct_words), np.array(es, dtype=np.int32)
    out, oe = np.full((45, ctx.ct_words), 0xA5A5A5A5, np.uint32), np.full(45, 77, np.int32)
    rc = ctx.lib.pai_mul_bcast(ctx.handle, ct.ctypes.data, ex.ctypes.data, 5, N.PAI_F64, x.ctypes.data, 9,
                               out.ctypes.data, oe.ctypes.data, None)
    assert rc == -5
    assert np.array_equal(out[:27], want[0][:27]) and np.array_equal(oe[:27], want[1][:27])
    assert (out[27:] == 0xA5A5A5A5).all() and (oe[27:] == 77).all()


@pytest.mark.parametrize("path", [0, 2])
def test_ciphertext_without_inverse(ctxs, path):
    N, ctx, key = _native(), ctxs[1024], _key(1024)
    cs, es = list(_cts(1024, 3)[0]), _cts(1024, 3)[1]
    cs[1] = key.p
    ct, ex = N.ints_to_words(cs, ctx.ct_words), np.array(es, dtype=np.int32)
    x = np.abs(_scalars(np.float64, 3, 9))
    x[0, 2] = -2.5                                          # a negative scalar in another row: fine
    out, oe, _ = _run(ctx, path, cs, es, x)
    assert _pairs(out, oe) == _oracle(1024, cs, es, x)
    x[1, 4] = -1.0
    out, oe, st = (np.full((27, ctx.ct_words), 0xA5A5A5A5, np.uint32), np.full(27, 77, np.int32), np.full(27, 77, np.int32))
    rc = ctx.lib.pai_mul_bcast(ctx.handle, ct.ctypes.data, ex.ctypes.data, 3, N.PAI_F64, x.ctypes.data, 9,
                               out.ctypes.data, oe.ctypes.data, st.ctypes.data)
    assert rc == -5                                         # PAI_ERR_NOINV, and nothing written
    assert (out == 0xA5A5A5A5).all() and (oe == 77).all() and (st == 77).all()


def test_statuses_and_options(ctxs):
    N, ctx = _native(), ctxs[1024]
    cs, es = _cts(1024, 2)
    x = _scalars(np.float64, 2, 9)
    x[0, 1], x[0, 5], x[1, 0] = np.nan, np.inf, -np.inf
    bad = np.isnan(x.reshape(-1)) | np.isinf(x.reshape(-1))
    for path in (0, 2):
        out, oe, st = _run(ctx, path, cs, es, x)
        assert np.array_equal(st, np.where(bad, N.EL_ENC_RANGE, 0))
        assert [p for p, b in zip(_pairs(out, oe), bad) if b] == [(1, es[0]), (1, es[0]), (1, es[1])]
    set_option = ctx.lib.pai_ctx_set_option
    assert set_option(ctx.handle, N.PAI_OPT_MUL_BCAST, 3) == -1 and set_option(ctx.handle, N.PAI_OPT_MUL_BCAST, -1) == -1
    assert set_option(ctx.handle, N.PAI_OPT_MUL_BCAST_PATH, 1) != 0
    assert ctx.mul_bcast_mode == 2 and ctx.mul_bcast_path == 2
    ct, ex = N.ints_to_words(list(cs), ctx.ct_words), np.array(es, dtype=np.int32)
    out, oe = np.empty((18, ctx.ct_words), np.uint32), np.empty(18, np.int32)
    args = (ct.ctypes.data, ex.ctypes.data, 2, N.PAI_BIG, x.ctypes.data, 9, out.ctypes.data, oe.ctypes.data, None)
    assert ctx.lib.pai_mul_bcast(ctx.handle, *args) == -1   # PAI_ERR_ARG


def test_package_layers():
    """`a * X` and `a[:, None] * X` on PaillierArray, CiphertextBuffer and DeviceCiphertextBuffer: the per-element
    operators' bits from exactly one pai_mul_bcast[_dev] call and no pai_mul call."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    pe, _ = generate_paillier_encryptor_decryptor(1024, seed=11)
    rng = np.random.default_rng(11)
    a = pe.encrypt(rng.standard_normal(6))
    plain = np.asarray(a)                                   # object ndarray: numpy's loop over __mul__
    ctx = _runtime.context(plain[0].public_key)
    host = CiphertextBuffer.from_array(a)
    dev = host.to_device()

    def bits(r):
        r = r.to_array() if hasattr(r, "to_array") else r
        return [(e.ciphertext(False), e.exponent) for e in np.asarray(r).reshape(-1)], np.shape(r)

    def counted(op):
        before = ctx.calls.copy()
        return bits(op()), ctx.calls - before

    for col, X in ((False, rng.standard_normal((4, 6))), (True, rng.integers(-9, 9, (6, 5)))):
        want = bits(plain[:, None] * X if col else plain * X)
        for obj, name in ((a, "pai_mul_bcast"), (host, "pai_mul_bcast"), (dev, "pai_mul_bcast_dev")):
            got, calls = counted(lambda: (obj[:, None] if col else obj) * X)
            assert got == want, (name, col)
            assert calls[name] == 1 and calls["pai_mul"] == 0 and calls["pai_mul_dev"] == 0, (name, calls)
    b = pe.encrypt(rng.standard_normal((4, 6)))
    m, x = CiphertextBuffer.from_array(b), rng.standard_normal(6)
    got, calls = counted(lambda: m * x)                     # buf(4, 6) * x(6,): only the plain side grows, pai_mul
    assert got == bits(np.asarray(b) * x)
    assert calls["pai_mul"] == 1 and calls["pai_mul_bcast"] == 0
    with pytest.raises((TypeError, ValueError)):
        host * np.ones((4, 5))
