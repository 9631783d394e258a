"""GPU parity of the bucket-method multi-exponentiation behind narrow matrix products (kernels_pip.hpp: k_pip_scan,
k_pip_plan, k_pip_acc, k_pip_red, k_pip_horner; PAI_OPT_MATMUL_BUCKET = 1): every output against the oracle
(mul_scalar / add_k, exact integers) and against the term path of the same context, bit-exact, and the calls outside its
class on the path they take without it."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (2, 5, 2), (1, 33, 1), (1, 70, 3), (3, 16, 15)]
PAI_ERR_NOINV = -5


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def k1024(golden):
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    ctx = _native().Context(key.n, 0)
    ctx.set_matmul_bucket(True)
    return ctx, key


@pytest.fixture(scope="module")
def spread(k1024):
    """120 oracle ciphertexts at 1024 bits of values spread over 1e-30 .. 1e30 (exponents 34 .. -16), never modified."""
    _, key = k1024
    rng = np.random.default_rng(120)
    vals = rng.standard_normal(120) * 10.0 ** rng.integers(-30, 31, 120)
    pairs = [O.encrypt_value(float(v), key, O.golden_r(key.n, 120, i)) for i, v in enumerate(vals)]
    return tuple(c for c, _ in pairs), tuple(e for _, e in pairs)


def _scalars(K, d, dt, lo=-6, hi=7):
    """Zeros, -0.0, +-1, +-2^62 (int64), float magnitudes 10^lo .. 10^hi; at (70, 3): a column of 3, one of -255."""
    rng = np.random.default_rng(7 * K + d)
    if dt == np.int64:
        x = rng.integers(-(2 ** 40), 2 ** 40, (K, d), dtype=np.int64)
        x.flat[1::7] = 2 ** 62
        x.flat[2::7] = -(2 ** 62)
    else:
        x = rng.standard_normal((K, d)) * 10.0 ** rng.integers(lo, hi, (K, d))
        x.flat[3::13] = -0.0
    x.flat[::5] = 0
    x.flat[1::9] = -1
    x.flat[4::11] = 1
    if (K, d) == (70, 3):
        x[:, 0], x[:, 1] = 3, -255
    return x.astype(dt)


def _same_as_oracle(ctx, key, cs, es, m, K, x, d, path):
    N = _native()
    out, oe = ctx.matmul(N.ints_to_words(list(cs), ctx.ct_words), np.array(es, dtype=np.int32), m, K, x, d)
    assert ctx.matmul_path == path
    py = (lambda v: int(v)) if x.dtype == np.int64 else (lambda v: x.dtype.type(v) if x.dtype == np.float32 else float(v))
    want = []
    for i in range(m):
        for j in range(d):
            t = [O.mul_scalar(cs[i * K + k], es[i * K + k], py(x[k, j]), key) for k in range(K)]
            want.append(O.add_k([c for c, _ in t], [e for _, e in t], key))
    assert list(zip(N.words_to_ints(out), (int(e) for e in oe))) == want


def test_option_and_report(k1024, spread):
    """Fails without the bucket path: the option is unknown there."""
    N = _native()
    assert N.PAI_OPT_MATMUL_BUCKET == 28
    ctx = N.Context(k1024[1].n, 0)
    assert not ctx.matmul_bucket
    ct, ex = N.ints_to_words(list(spread[0][:64]), ctx.ct_words), np.array(spread[1][:64], dtype=np.int32)
    x = _scalars(64, 1, np.float64)
    a, ae = ctx.matmul(ct, ex, 1, 64, x, 1)
    assert ctx.matmul_path == 1
    ctx.set_matmul_bucket(True)
    assert ctx.matmul_bucket
    b, be = ctx.matmul(ct, ex, 1, 64, x, 1)
    assert ctx.matmul_path == 3
    assert np.array_equal(a, b) and np.array_equal(ae, be)
    assert ctx.lib.pai_ctx_set_option(ctx.handle, N.PAI_OPT_MATMUL_PATH, 3) != 0   # read-only


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("m,K,d", SHAPES)
def test_vs_oracle(k1024, spread, m, K, d, dt):
    """Every output: one term, K below and above a run of 32 members, a bucket of 70 members (three runs), the top bucket
    on the negative side alone, 45 outputs; ciphertext exponents spread over 50 digits, so up to 66 windows of 4 bits (effective exponents of at most 261 bits, computed with the oracle's encoder)."""
    ctx, key = k1024
    _same_as_oracle(ctx, key, spread[0][:m * K], spread[1][:m * K], m, K, _scalars(K, d, dt), d, 3)


def _bucket_equals_term_path(ctx, m, K, d, seed):
    """Device-encrypted ciphertexts (explicit small obfuscators) of values over 1e-30 .. 1e30, float64 and int64 scalars."""
    N = _native()
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal(m * K) * 10.0 ** rng.integers(-30, 31, m * K)
    ct, ex, st = ctx.encrypt(vals, obf_mode=N.PAI_OBF_GIVEN, r=[int(v) for v in rng.integers(2, 2 ** 62, m * K)])
    assert np.all(st == 0)
    for dt in (np.float64, np.int64):
        x = _scalars(K, d, dt)
        ctx.set_matmul_bucket(True)
        out, oe = ctx.matmul(ct, ex, m, K, x, d)
        assert ctx.matmul_path == 3
        ctx.set_matmul_bucket(False)
        ref, re_ = ctx.matmul(ct, ex, m, K, x, d)
        assert ctx.matmul_path == 1
        assert np.array_equal(out, ref) and np.array_equal(oe, re_)


def test_bucket_equals_term_path_2048(golden):
    """4 lanes per group."""
    _bucket_equals_term_path(_native().Context(int(golden["keys"]["2048"]["n"], 16), 0), 3, 100, 5, 2048)


def test_bucket_equals_term_path_3072():
    """8 lanes per group: the seeded 3072-bit key of test_gpu_ops_sizes.py."""
    seed = 2
    while True:
        p, q = O.getprimeover(1536, seed=seed), O.getprimeover(1536, seed=seed + 1000)
        if p != q and (p * q).bit_length() == 3072:
            break
        seed += 1
    _bucket_equals_term_path(_native().Context(p * q, 0), 2, 20, 3, 3072)


@pytest.mark.parametrize("K", [120, 300, 900])
def test_every_window_width(golden, K):
    """K selects the window: 5, 6 and 8 bits (4 in the cases above). At 8 bits the 38 windows of these exponents take
    76 KiB of counters, more than a launch gets without asking."""
    _bucket_equals_term_path(_native().Context(int(golden["keys"]["1024"]["n"], 16), 0), 1, K, 1, K)


def test_not_invertible(k1024, spread):
    """A ciphertext that shares a factor with n: PAI_ERR_NOINV with nothing written once its scalar is negative, the
    oracle's bits under a positive scalar with a negative one elsewhere."""
    N = _native()
    ctx, key = k1024
    cs, es = list(spread[0][:5]), list(spread[1][:5])
    cs[2] = key.p
    x = np.array([[1.0, 2.0], [0.5, 3.0], [2.0, 7.0], [4.0, -1.0], [5.0, 6.0]])
    _same_as_oracle(ctx, key, cs, es, 1, 5, x, 2, 3)
    x[2, 0] = -2.0
    ct, ex = N.ints_to_words(cs, ctx.ct_words), np.array(es, dtype=np.int32)
    out = np.full((2, ctx.ct_words), 0xA5A5A5A5, dtype=np.uint32)
    oe = np.full(2, -77, dtype=np.int32)
    rc = ctx.lib.pai_matmul(ctx.handle, N._ptr(ct), N._ptr(ex), 1, 5, N.scalar_dtype(x), N._ptr(x), 2, N._ptr(out), N._ptr(oe))
    assert rc == PAI_ERR_NOINV and ctx.matmul_path == 3
    assert np.all(out == 0xA5A5A5A5) and np.all(oe == -77)


def test_outside_the_class(k1024, spread):
    """Scalars over 10^+-300 need about 2000 bits of effective exponent, above the cap of 512: the term path. 16 columns:
    the path of a context without the option (too few terms for the fused path: the term path)."""
    ctx, key = k1024
    _same_as_oracle(ctx, key, spread[0][:12], spread[1][:12], 1, 12, _scalars(12, 2, np.float64, -300, 301), 2, 1)
    _same_as_oracle(ctx, key, spread[0][:6], spread[1][:6], 1, 6, _scalars(6, 16, np.float64), 16, 1)


def test_package_dot(monkeypatch):
    """FLEXPAI_MATMUL_BUCKET=1 is read when the key's context is created."""
    monkeypatch.setenv("FLEXPAI_MATMUL_BUCKET", "1")
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    pe, _ = generate_paillier_encryptor_decryptor(1024, seed=28)
    enc = pe.encrypt(np.array([0.5, -1.25, 3.0e-3, 0.0, 1234.5678, -7.0]))
    feats = _scalars(6, 2, np.float64)
    got = enc.dot(feats)
    plain = np.asarray(enc)
    key = O.Key(plain[0].public_key.n)
    assert [c.matmul_path for c in _runtime.cached_contexts() if c.n == key.n] == [3]
    for j in range(2):
        t = [O.mul_scalar(c.ciphertext(False), c.exponent, float(feats[k, j]), key) for k, c in enumerate(plain)]
        assert (got[j].ciphertext(False), got[j].exponent) == O.add_k([c for c, _ in t], [e for _, e in t], key)
