"""GPU parity of the plain scalar operand at the encoder's edges (tests/scalar_edges.py): what k_mul, k_plain, k_mm_sign,
k_mm_acc, k_sd_sign and k_sd_acc do with the (M, e) of int64 scalars that use bit 63, floats on both sides of the 1e-200
cut, denormals, the largest doubles and floats, NaN and +-inf, through pai_mul, pai_add_plain, pai_matmul and
pai_segment_dot at 2, 4 and 8 lanes and through the package at 1024 bits. Bit-exact, every output.

Every expected value is the oracle's (mul_scalar, add_scalar, add_k), or the documented rule for a scalar that does not
encode applied to oracle terms: the factor 1 at exponent exp_i + 0 with PAI_EL_ENC_RANGE (include/flexpai.h). The package
is held against numpy's per-object loop over PaillierEncryptedNumber, which test_scalar_edges_cpu.py holds against the
oracle. The fused paths of pai_matmul and pai_segment_dot run on the test build under $FLEXPAI_MM_ALWAYS=1 and
$FLEXPAI_SD_ALWAYS=1, the term paths through set_matmul_fused(False) / set_segdot_fused(False); the two are compared with
each other in addition to the oracle."""
import functools

import numpy as np
import pytest

import scalar_edges as SE
from oracle import paillier_oracle as O
from test_gpu_ops_sizes import _make_key, _rand_cts

pytestmark = pytest.mark.gpu
KEYS = ["K1024", "K2071", "K4096"]
FLOATS = [np.float64, np.float32]
NCT = 64
TOP = 7                                  # the ciphertext with the largest exponent (9; the others lie in -6 .. 6)


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(autouse=True)
def _always_fused(monkeypatch):
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")          # read by the test build only, at every call
    monkeypatch.setenv("FLEXPAI_SD_ALWAYS", "1")
    monkeypatch.delenv("FLEXPAI_MM_TABLE_BYTES", raising=False)
    monkeypatch.delenv("FLEXPAI_SD_SLICE", raising=False)


class _Operands:
    """Per key: a public-only context on the test build, the oracle's key, 64 random residues below n^2 as ciphertexts
    and their exponents. Made on first use, kept for the module, never modified."""

    def __init__(self, golden, xlib):
        self.golden, self.xlib, self.made = golden, xlib, {}

    def __call__(self, name):
        if name not in self.made:
            if name == "K1024":
                k = self.golden["keys"]["1024"]
                key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
            else:
                key = _make_key(name, self.golden)
            N = _native()
            ctx = N.Context(key.n, 0, lib=self.xlib)
            rng = np.random.default_rng(key.n.bit_length() + 63)
            cs = _rand_cts(rng, key, NCT)
            ex = rng.integers(-6, 7, NCT).astype(np.int32)
            ex[TOP] = 9
            self.made[name] = (ctx, key, tuple(cs), N.ints_to_words(cs, ctx.ct_words), ex)
        return self.made[name]


@pytest.fixture(scope="module")
def operands(golden, xlib):
    return _Operands(golden, xlib)


def _lists(name):
    """The (dtype, scalars) of a key: everything at 2 and 4 lanes; at 4096 bits, where the oracle's 8192-bit pow
    dominates, the int64 list and the six-float subset."""
    if name == "K4096":
        return [(np.int64, SE.scalars(np.int64)), (np.float64, np.array(SE.F64_SUBSET))]
    return [(dt, SE.scalars(dt)) for dt in (np.int64, np.float64, np.float32)]


def _pairs(out, oe):
    return list(zip(_native().words_to_ints(out), (int(e) for e in oe)))


# --------------------------------------------------------------------------- pai_mul
@pytest.mark.parametrize("name", KEYS)
def test_mul(operands, name):
    """A dtype's whole list in one call: 0-window, 1-window and 16-window scalars and the ones that do not encode share
    a wave. Then INT64_MIN (|M| = 2^63: digit 8 of window 15), INT64_MAX and -DBL_MAX as the one scalar of a call."""
    ctx, key, cs, words, ex = operands(name)
    for dt, x in _lists(name):
        n = len(x)
        out, oe, st = ctx.mul(words[:n], ex[:n], x)
        got = _pairs(out, oe)
        for i in range(n):
            s = SE.py(x[i], dt)
            print(name, np.dtype(dt).name, repr(s), int(st[i]), got[i][1])
            if SE.finite(s):
                assert int(st[i]) == 0 and got[i] == SE.expect_mul(cs[i], int(ex[i]), s, key), (dt, s)
            else:
                assert (int(st[i]), got[i]) == (SE.EL_ENC_RANGE, (1, int(ex[i]))), (dt, s)
    for x in (np.array([SE.INT64_MIN], dtype=np.int64), np.array([SE.INT64_MAX], dtype=np.int64), np.array([-SE.DBL_MAX])):
        out, oe, st = ctx.mul(words[:3], ex[:3], x)          # x_stride = 0
        s = SE.py(x[0], x.dtype.type)
        assert not st.any()
        assert _pairs(out, oe) == [SE.expect_mul(cs[i], int(ex[i]), s, key) for i in range(3)], s


# --------------------------------------------------------------------------- pai_add_plain
@pytest.mark.parametrize("name", KEYS)
def test_add_plain(operands, name):
    """Every scalar on ciphertext exponents around its own (both branches of encode_plain_max), far below, and at 255.
    A finite scalar: the oracle's bits, PAI_EL_FLOAT_OVF where it raises OverflowError, PAI_EL_ENC_RANGE where it raises
    ValueError. NaN: PAI_EL_ENC_RANGE; +-inf: PAI_EL_FLOAT_OVF; never status 0."""
    ctx, key, cs, words, _ = operands(name)
    for dt, x in _lists(name):
        cases = [(v, me) for v in x for me in SE.add_plain_exps(SE.py(v, dt), dt, key)]
        for lo in range(0, len(cases), NCT):
            part = cases[lo:lo + NCT]
            n = len(part)
            xs = np.array([v for v, _ in part], dtype=dt)
            me = np.array([e for _, e in part], dtype=np.int32)
            out, oe, st = ctx.add_plain(words[:n], me, xs)
            got = _pairs(out, oe)
            for i, (v, e) in enumerate(part):
                s = SE.py(v, dt)
                want_st, want = SE.expect_add_status(cs[i], e, s, key)
                print(name, np.dtype(dt).name, repr(s), e, int(st[i]), want_st)
                assert int(st[i]) == want_st, (dt, s, e)
                if want_st == 0:
                    assert got[i] == want, (dt, s, e)


# --------------------------------------------------------------------------- pai_matmul
M_, K_, D_ = 2, 17, 3


def _both_mm(ctx, words, ex, x):
    out, oe = ctx.matmul(words[:M_ * K_], ex[:M_ * K_], M_, K_, x, D_)
    assert ctx.matmul_path == 2
    ctx.set_matmul_fused(False)
    try:
        ref, re_ = ctx.matmul(words[:M_ * K_], ex[:M_ * K_], M_, K_, x, D_)
        assert ctx.matmul_path == 1
    finally:
        ctx.set_matmul_fused(True)
    return _pairs(out, oe), _pairs(ref, re_)


def _cycle(vals, count, start=0):
    return [vals[(start + i) % len(vals)] for i in range(count)]


def _zero_class(dt):
    """The floats that encode as the int 0."""
    return [v for v in SE.scalars(dt, finite_only=True) if abs(float(v)) < SE.CUT]


def _low_class(dt):
    """Floats whose terms cannot hold a sum's largest exponent next to a ciphertext at exponent 9: the int-0 class
    (e = 0) and the largest magnitudes (e = -243, -19)."""
    big = SE.DBL_MAX if dt == np.float64 else SE.FLT_MAX
    return _zero_class(dt) + [big, -big]


@pytest.mark.parametrize("name", KEYS)
def test_matmul_finite(operands, name):
    """(2 x 17) by (17 x 3), two chunks of 16 and 1, on both paths: the finite list fills x; for floats column 1 holds
    only the int-0 class (the value 1 at the operands' largest exponent), for int64 row 5 holds INT64_MIN in every
    column."""
    ctx, key, cs, words, ex = operands(name)
    for dt, vals in _lists(name):
        fin = [v for v in vals if SE.finite(SE.py(v, dt))]
        x = np.array(_cycle(fin, K_ * D_), dtype=dt).reshape(K_, D_)
        if dt == np.int64:
            x[5, :] = SE.INT64_MIN
        else:
            # +-1e-200 (e = 179) in column 0 only and +-DBL_MAX (e = -243) in column 2 only: every scalar meets every
            # kernel, and the oracle raises one column's terms by 16^190, not all three by 16^430
            x[:, 0] = _cycle([v for v in fin if abs(float(v)) != SE.DBL_MAX], K_)
            x[:, 1] = _cycle([v for v in fin if abs(float(v)) < SE.CUT], K_)
            x[:, 2] = _cycle([v for v in fin if abs(float(v)) != SE.CUT], K_)
        fused, term = _both_mm(ctx, words, ex, x)
        want = SE.expect_dot(cs, ex, M_, K_, x, D_, key)
        assert fused == want, dt
        assert term == want, dt
        if dt != np.int64:
            for i in range(M_):
                assert want[i * D_ + 1] == (1, int(ex[i * K_:(i + 1) * K_].max()))


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("name", ["K1024", "K2071"])
def test_matmul_non_finite(operands, name, dt):
    """One NaN and one infinity in different columns whose other scalars have exponents <= 0, so the exponent the
    library gives the factor 1 decides the sum's: both paths give the factor-1 expectation, and column 1 (finite) is the
    oracle's."""
    ctx, key, cs, words, ex = operands(name)
    fin = list(SE.scalars(dt, finite_only=True))
    x = np.empty((K_, D_), dtype=dt)
    x[:, 0] = _cycle(_low_class(dt), K_)
    x[:, 1] = _cycle(fin, K_)
    x[:, 2] = _cycle(_low_class(dt), K_, 3)
    x[3, 0] = SE.NAN
    x[16, 2] = -SE.INF                                     # the lone operand of the second chunk
    fused, term = _both_mm(ctx, words, ex, x)
    want = SE.expect_dot(cs, ex, M_, K_, x, D_, key, factor_one=True)
    print(name, np.dtype(dt).name, [e for _, e in fused], [e for _, e in term], [e for _, e in want])
    assert fused == term
    assert fused == want
    col1 = SE.expect_dot(cs, ex, M_, K_, np.ascontiguousarray(x[:, 1:2]), 1, key)
    assert [fused[i * D_ + 1] for i in range(M_)] == col1


# --------------------------------------------------------------------------- pai_segment_dot
LENS = (0, 1, 16, 17)


def _run_sd(ctx, fused, *args):
    ctx.set_segdot_fused(fused)
    try:
        out, oe, st = ctx.segment_dot(*args)
        assert ctx.segdot_path == (2 if fused else 1)
    finally:
        ctx.set_segdot_fused(True)
    return _pairs(out, oe), st


def _sd_index(name):
    rng = np.random.default_rng(len(name) + 34)
    idx = rng.integers(0, NCT, sum(LENS)).astype(np.int64)
    idx[idx == TOP] = TOP + 1
    idx[3] = idx[2]                                        # a ciphertext repeated inside a chunk
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    return idx, off


@pytest.mark.parametrize("name", KEYS)
def test_segment_dot_finite(operands, name):
    ctx, key, cs, words, ex = operands(name)
    idx, off = _sd_index(name)
    for dt, vals in _lists(name):
        fin = [v for v in vals if SE.finite(SE.py(v, dt))]
        x = np.array(_cycle(fin, idx.size), dtype=dt)
        want = SE.expect_segdot(cs, ex, idx, off, x, key)
        for fused in (True, False):
            got, st = _run_sd(ctx, fused, words, ex, idx, off, x)
            assert not st.any(), (dt, fused)
            assert got == want, (dt, fused)


@pytest.mark.parametrize("dt", FLOATS)
@pytest.mark.parametrize("name", ["K1024", "K2071"])
def test_segment_dot_non_finite(operands, name, dt):
    """A NaN as the only entry of a segment; an infinity on the ciphertext with the largest exponent of the 16-entry
    segment, whose other scalars have exponents <= 0; -inf as the lone entry of the 17-entry segment's second chunk.
    pai_mul's statuses, the factor-1 bits, on both paths."""
    ctx, key, cs, words, ex = operands(name)
    idx, off = _sd_index(name)
    fin = list(SE.scalars(dt, finite_only=True))
    x = np.array(_cycle(fin, idx.size), dtype=dt)
    x[1:17] = _cycle(_low_class(dt), 16)
    bad = {0: SE.NAN, 6: SE.INF, 33: -SE.INF}
    idx[6] = TOP
    for t, v in bad.items():
        x[t] = v
    assert max(int(ex[i]) for i in idx[1:17]) == int(ex[TOP]) == 9
    want = SE.expect_segdot(cs, ex, idx, off, x, key, factor_one=True)
    assert want[1] == (1, int(ex[idx[0]])) and want[2][1] == 9
    want_st = [SE.EL_ENC_RANGE if t in bad else 0 for t in range(idx.size)]
    res = {}
    for fused in (True, False):
        res[fused], st = _run_sd(ctx, fused, words, ex, idx, off, x)
        print(name, np.dtype(dt).name, fused, [e for _, e in res[fused]], [e for _, e in want], list(st))
        assert list(st) == want_st, fused
    assert res[True] == res[False]
    assert res[True] == want


# --------------------------------------------------------------------------- the package, 1024 bits
class _Csc:
    """What the package relies on of a sparse operand: .tocsc() and, on its result, indptr / indices / data / shape."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = np.array(indptr), np.array(indices), np.asarray(data), shape

    def tocsc(self):
        return self


@pytest.fixture(scope="module")
def pkg():
    """(PaillierArray of 18 encryptions, the same as a plain object array, the same as a CiphertextBuffer)."""
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    pe, _ = generate_paillier_encryptor_decryptor(1024, seed=63)
    enc = pe.encrypt(np.random.default_rng(63).standard_normal(18))
    return enc, np.asarray(enc), CiphertextBuffer.from_array(enc)


def _bits(r):
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    if isinstance(r, CiphertextBuffer):
        r = r.to_array()
    flat = np.asarray(r, dtype=object).reshape(-1) if isinstance(r, np.ndarray) else [r]
    return [(e.ciphertext(False), e.exponent) if hasattr(e, "ciphertext") else e for e in flat]


def _agree(got_fn, want_fn, what):
    """The per-object loop's bits, or its exception class with no result."""
    try:
        want = want_fn()
    except (ValueError, OverflowError) as err:
        with pytest.raises(type(err)):
            got_fn()
        return False
    assert _bits(got_fn()) == _bits(want), what
    return True


def _loop_dot(plain, rows, ws):
    """sum of plain[i] * w over the stored entries, by the per-object operators (no `0 +`)."""
    return functools.reduce(lambda a, b: a + b, [plain[int(i)] * w for i, w in zip(rows, ws)])


@pytest.mark.parametrize("dt", [np.int64, np.float64, np.float32])
def test_package_finite(pkg, dt):
    """Each finite edge scalar through * and + (as a scalar and inside an array), dot, @ csc, segment_dot and the
    CiphertextBuffer counterparts: the bits of numpy's per-object loop, or its exception (an addend of 2^1024 is past
    max_int at this key size) raised by the whole operation."""
    from flex.crypto.paillier import parallel_ops
    enc, plain, buf = pkg
    x = SE.scalars(dt, finite_only=True)
    n = len(x)
    e, p, b = enc[:n], plain[:n], buf[:n]
    compared = 0
    for v in x:
        s = SE.py(v, dt)
        for got, want, what in ((lambda: e[:2] * s, lambda: p[:2] * s, "array * scalar"),
                                (lambda: b[:2] * s, lambda: p[:2] * s, "buffer * scalar"),
                                (lambda: e[:2] + s, lambda: p[:2] + s, "array + scalar"),
                                (lambda: b[:2] + s, lambda: p[:2] + s, "buffer + scalar")):
            compared += _agree(got, want, (what, s))
    assert compared >= 4 * (n - 2)
    assert _agree(lambda: e * x, lambda: p * x, "array * array") and _agree(lambda: b * x, lambda: p * x, "buffer * array")
    _agree(lambda: e + x, lambda: p + x, "array + array")
    _agree(lambda: b + x, lambda: p + x, "buffer + array")
    addable = np.array([i for i in range(n) if not isinstance(
        SE.expect_add(p[i].ciphertext(False), p[i].exponent, SE.py(x[i], dt), O.Key(p[i].public_key.n)), type)])
    assert addable.size >= n - 2
    assert _agree(lambda: e[addable] + x[addable], lambda: p[addable] + x[addable], "array + array")
    assert _agree(lambda: b[addable] + x[addable], lambda: p[addable] + x[addable], "buffer + array")
    # sums: a term at exponent e_i + e(x) is raised to the sum's largest exponent through __mul__(16^gap), which the
    # reference refuses past max_int (gap >= 256 at this key). +-DBL_MAX (e = -243) therefore meets only the int-0 class
    # (xb); every other scalar, +-1e-200 (e = 179) among them, is in xa
    xa, xb = x.copy(), x.copy()
    if dt == np.float64:
        xa[np.abs(xa) == SE.DBL_MAX] = 0.1
        xb[(np.abs(xb) >= SE.CUT) & (np.abs(xb) < SE.DBL_MAX)] = 0.0
        assert (np.abs(xa) == SE.CUT).sum() == 2 and (np.abs(xb) == SE.DBL_MAX).sum() == 2
    X = np.stack([xa, xb, np.roll(xb, 3)], axis=1)
    assert _agree(lambda: e.dot(X), lambda: p.dot(X), "array . matrix") and _agree(lambda: b.dot(X), lambda: p.dot(X), "buffer . matrix")
    assert _agree(lambda: e.dot(xa), lambda: p.dot(xa), "array . vector") and _agree(lambda: b @ xa, lambda: p.dot(xa), "buffer @ vector")
    # a sparse (n, 2) matrix: column 0 stores every row, column 1 the rows 1, 3, 5, ..
    odd = list(range(1, n, 2))
    data = np.concatenate([xa, xb[odd]])
    csc = _Csc([0, n, n + len(odd)], list(range(n)) + odd, data, (n, 2))
    want = [_loop_dot(p, range(n), [SE.py(v, dt) for v in xa]), _loop_dot(p, odd, [SE.py(v, dt) for v in xb[odd]])]
    assert _bits(e @ csc) == _bits(np.array(want, dtype=object)) == _bits(b @ csc)
    seg = b.segment_dot(list(range(n)) + odd, [0, n, n + len(odd)], data)
    assert _bits(seg) == _bits(np.array(want, dtype=object))
    res = parallel_ops.segment_dot(p, [list(range(n)), [], odd], [xa, xa[:0], xb[odd]])
    assert res[1] == 0 and _bits(np.array([res[0], res[2]], dtype=object)) == _bits(np.array([0 + w for w in want], dtype=object))


@pytest.mark.parametrize("where", ["only", "first", "last"])
@pytest.mark.parametrize("bad,exc", [(SE.NAN, ValueError), (SE.INF, OverflowError), (-SE.INF, OverflowError)])
@pytest.mark.parametrize("dt", FLOATS)
def test_package_non_finite_raises(pkg, dt, bad, exc, where):
    """NaN and +-inf as the only, the first and the last element of a plain operand: every operation raises what
    numpy's per-object loop raises, as a whole."""
    from flex.crypto.paillier import parallel_ops
    enc, plain, buf = pkg
    good = [1.5, -2.0, 0.25]
    x = np.array({"only": [bad], "first": [bad] + good, "last": good + [bad]}[where], dtype=dt)
    n = len(x)
    e, p, b = enc[:n], plain[:n], buf[:n]
    s = SE.py(dt(bad), dt)
    X = np.stack([np.ones(n, dtype=dt), x], axis=1)
    csc = _Csc([0, n], list(range(n)), x, (n, 1))
    rows = list(range(n))
    for loop in (lambda: p * x, lambda: p + x, lambda: p * s, lambda: p + s, lambda: p.dot(x), lambda: p.dot(X)):
        with pytest.raises(exc):                           # the per-object loop itself
            loop()
    ops = {"array * array": lambda: e * x, "array + array": lambda: e + x, "array * scalar": lambda: e * s,
           "array + scalar": lambda: e + s, "scalar * array": lambda: s * e, "array . vector": lambda: e.dot(x),
           "array . matrix": lambda: e.dot(X), "array @ csc": lambda: e @ csc,
           "parallel_ops.mul": lambda: parallel_ops.mul(p, x), "parallel_ops.add": lambda: parallel_ops.add(p, x),
           "parallel_ops.segment_dot": lambda: parallel_ops.segment_dot(p, [rows], [x]),
           "buffer * array": lambda: b * x, "buffer + array": lambda: b + x, "buffer * scalar": lambda: b * s,
           "buffer + scalar": lambda: b + s, "buffer . vector": lambda: b.dot(x), "buffer . matrix": lambda: b.dot(X),
           "buffer @ csc": lambda: b @ csc, "buffer.segment_dot": lambda: b.segment_dot(rows, [0, n], x)}
    wrong = []
    for what, op in ops.items():
        try:
            r = op()
        except exc:
            continue
        except Exception as err:   # noqa: BLE001 - reported with the operation's name
            wrong.append(f"{what} raised {type(err).__name__}")
        else:
            wrong.append(f"{what} returned a {type(r).__name__}")
    assert not wrong, f"the per-object loop raises {exc.__name__}: {wrong}"
