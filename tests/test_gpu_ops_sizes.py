"""GPU parity of the homomorphic operators (pai_add, pai_mul, pai_add_plain, pai_matmul on the term path,
pai_segment_add: k_add, k_mul, k_plain, k_inv_up / k_inv_down) against the oracle (add_k, mul_scalar, add_scalar) at
every lane-group size and at the seams between them, bit-exact, every output:

  K512   n of 512 bits   groups of 2   n^2 fills half the limbs
  K1035  1035 bits       2             the largest 2-lane key: 2 nb + 2 = 28 * 74, ct_words 65 reaches past limb 73
  K1036  1036 bits       4             the smallest 4-lane key
  K2071  2071 bits       4             the largest 4-lane key: ct_words 130 reaches past limb 147
  K2072  2072 bits       8             the smallest 8-lane key
  K3072  3072 bits       8
  K4096  4096 bits       8             the golden key

and, at the 1024-bit golden key, the parts of the operators no other test reaches: sums of more than ADD_KMAX = 64
operands (add_dev's split), the R^64 Montgomery corrections, the clamped schedule bucket of k_add_plan, and the batch
inversion's segment lengths 5, 17 and 64 with ragged last segments. The k_plain cases walk the shifted multiplier
|M| = mag 2^sh across the limbs of every lane a multiplier below 2^(nb - 3) can start in, over the lane seams, and up to
the range check's boundary.

The oracle works on Python integers and does not depend on the key size; the reference's goldens pin it
(tests/test_oracle_*_golden.py). Ciphertext operands are random integers below n^2 (a non-unit has negligible
probability); at K3072 and K4096 a few real encryptions also go through a sum and the key holder's decryption."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
INT32_MIN = int(np.iinfo(np.int32).min)
LIMB_BITS, LANE_LIMBS = 28, 37                      # bn_group.hpp: LB, L
# name -> (bits of n, bits of the two primes, first seed tried, lanes per group)
GENERATED = {"K1035": (1035, 518, 517, 1, 2), "K1036": (1036, 518, 518, 1, 4), "K2071": (2071, 1036, 1035, 1, 4),
             "K2072": (2072, 1036, 1036, 1, 8), "K3072": (3072, 1536, 1536, 2, 8)}
LANES = {"K512": 2, "K4096": 8, **{k: v[4] for k, v in GENERATED.items()}}
ALL_KEYS = ["K512", "K1035", "K1036", "K2071", "K2072", "K3072", "K4096"]


def _native():
    from flex.crypto.paillier import _native
    return _native


def _prime_below(x):
    """The largest prime below x, stepping down with the oracle's Miller-Rabin."""
    x -= 1
    while not O._is_probable_prime(x):
        x -= 1
    return x


# Top-heavy keys: name -> (bits of n, bits below which p is the largest prime, the same for q). Equal bounds: q is the
# largest prime below p. n = p q lies just under 2^nb, so n^2 (or p^2) sits within a hair of the power of two above it.
TOP_HEAVY = {"K1034T": (1034, 517, 517), "K1035T": (1035, 518, 517), "K2048T": (2048, 1024, 1024),
             "K2071T": (2071, 1036, 1035)}


def _make_key(name, golden):
    if name in TOP_HEAVY:
        nb, pb, qb = TOP_HEAVY[name]
        p = _prime_below(1 << pb)
        q = _prime_below(p if qb == pb else 1 << qb)
        assert (p * q).bit_length() == nb
        return O.Key(p * q, p, q)
    if name == "K512":
        k = next(e for e in golden["keygen"] if e["nb"] == 512 and e["seed"] == 99)
        return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    if name == "K4096":
        k = golden["keys"]["4096"]
        return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    nb, pb, qb, seed, _ = GENERATED[name]
    while True:                                      # step the seed until n has exactly nb bits
        p, q = O.getprimeover(pb, seed=seed), O.getprimeover(qb, seed=seed + 1000)
        if p != q and (p * q).bit_length() == nb:
            return O.Key(p * q, p, q)
        seed += 1


class _Keys:
    """Keys and public-only contexts on the product library, made on first use and kept for the module."""

    def __init__(self, golden):
        self.golden, self.made = golden, {}

    def __call__(self, name):
        if name not in self.made:
            key = _make_key(name, self.golden)
            self.made[name] = (_native().Context(key.n, 0), key)
        return self.made[name]


@pytest.fixture(scope="module")
def keys(golden):
    return _Keys(golden)


@pytest.fixture(scope="module")
def k1024(golden):
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    return _native().Context(key.n, 0), key


def _rand_cts(rng, key, count):
    nbytes = (key.nsquare.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rng.bytes(nbytes), "little") % key.nsquare for _ in range(count)]


def _same(out, oe, want, what):
    """Every output: the ciphertext integer and the exponent."""
    got = list(zip(_native().words_to_ints(out), (int(e) for e in oe)))
    assert len(got) == len(want), what
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{what}: {len(bad)} of {len(want)} outputs differ from the oracle, first at {bad[:8]}"


def _py(v, dt):
    return int(v) if dt == np.int64 else (np.float32(v) if dt == np.float32 else float(v))


@pytest.mark.parametrize("name", ALL_KEYS)
def test_key_shapes(keys, name):
    ctx, key = keys(name)
    nb = key.n.bit_length()
    want_nb = {"K512": 512, "K4096": 4096}.get(name) or GENERATED[name][0]
    assert nb == want_nb and ctx.key_bits == nb
    assert ctx.ct_words == (2 * nb + 31) // 32 and ctx.pt_words == (nb + 31) // 32
    # the lane group the engine picks for n^2 (flexpai.hip tpi_for_bits: the smallest of 2, 4, 8 with 28 * 37 * TPI >=
    # 2 nb + 2), and the seams: at 1035 and 2071 bits 2 nb + 2 fills the group's limbs exactly
    tpi = next(t for t in (2, 4, 8) if LIMB_BITS * LANE_LIMBS * t >= 2 * nb + 2)
    assert tpi == LANES[name]
    if name in ("K1035", "K2071"):
        assert 2 * nb + 2 == LIMB_BITS * LANE_LIMBS * tpi and 32 * ctx.ct_words > LIMB_BITS * LANE_LIMBS * tpi


# --------------------------------------------------------------------------- add
ADD_N = (1, 31, 33, 70)     # ragged against the 32 groups per block of the 8-lane engine and the 64 of the 4-lane one


def _add_exps(rng, k, n):
    """[k][n] exponents in -20 .. 40. Of every 14 columns one is strictly increasing over the operands, one strictly
    decreasing and one independent over the whole range (column 0, the call of one instance, among them); three have all
    operands equal, the others lie within three neighbouring levels. The oracle's cost is in the wide columns (one
    c^(16^gap) per operand, about 0.2 s per 16-operand column at 4096 bits), hence no more of them."""
    e = np.empty((k, n), dtype=np.int32)
    for c in range(n):
        kind = c % 14
        if kind in (0, 5) and k > 1:
            step = int(rng.integers(1, 60 // (k - 1) + 1))
            col = int(rng.integers(-20, 41 - step * (k - 1))) + step * np.arange(k)
            e[:, c] = col if kind == 0 else col[::-1]
        elif kind == 9:
            e[:, c] = rng.integers(-20, 41, k)
        elif kind in (2, 7, 12):
            e[:, c] = rng.integers(-20, 41)
        else:
            e[:, c] = rng.integers(-20, 39) + rng.integers(0, 3, k)
    assert e.min() >= -20 and e.max() <= 40
    return e


@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ALL_KEYS)
def test_add_vs_oracle(keys, name, k):
    """One set of 70 columns; the calls of 1, 31, 33 and 70 instances take its first columns, so the oracle runs once."""
    N = _native()
    ctx, key = keys(name)
    rng = np.random.default_rng(1000 * k + key.n.bit_length())
    nmax = max(ADD_N)
    cs = [_rand_cts(rng, key, nmax) for _ in range(k)]
    ex = _add_exps(rng, k, nmax)
    want = [O.add_k([cs[j][i] for j in range(k)], [int(ex[j, i]) for j in range(k)], key) for i in range(nmax)]
    words = [N.ints_to_words(c, ctx.ct_words) for c in cs]
    for n in ADD_N:
        out, oe = ctx.add([w[:n] for w in words], [ex[j, :n] for j in range(k)])
        _same(out, oe, want[:n], f"add {name} k={k} N={n}")


@pytest.mark.parametrize("name", ["K3072", "K4096"])
def test_sum_of_encryptions_decrypts(keys, name):
    """Real ciphertexts (the oracle's encrypt_value) through a 3-way sum at 8 lanes, then the key holder's decryption:
    the sum's bits and the decoded float are the oracle's."""
    N = _native()
    _, key = keys(name)
    holder = N.Context(key.n, 0, key.p, key.q)
    vals = [[0.75, -1234.5], [-2.0e-9, 3.0], [1.0e6, 0.015625]]           # exponents differ across the operands
    enc = [[O.encrypt_value(v, key, O.golden_r(key.n, 31, 2 * j + i)) for i, v in enumerate(row)]
           for j, row in enumerate(vals)]
    want = [O.add_k([enc[j][i][0] for j in range(3)], [enc[j][i][1] for j in range(3)], key) for i in range(2)]
    out, oe = holder.add([N.ints_to_words([c for c, _ in row], holder.ct_words) for row in enc],
                         [np.array([e for _, e in row], dtype=np.int32) for row in enc])
    _same(out, oe, want, f"add {name}")
    val, _, st, _ = holder.decrypt(out, oe)
    assert np.all(st == 0)
    for i, (c, e) in enumerate(want):
        assert float(val[i]) == float(O.decrypt_value(c, e, key)), i
        assert float(val[i]) == pytest.approx(sum(row[i] for row in vals), rel=1e-12)


# --------------------------------------------------------------------------- mul
MUL_N = (1, 33, 70)


def _mul_scalars(rng, count, dt):
    """The mix of test_gpu_mul.py::test_mul_vs_oracle_mixed_scalars, with 1-window (+-1) and 16-window (+-2^62)
    exponents next to each other in one wave."""
    if dt == np.int64:
        x = rng.integers(-(2 ** 62), 2 ** 62, count, dtype=np.int64)
        x[::4] = 0
        x[1::8] = -1
        x[2::8] = 2 ** 62
        x[5::8] = -(2 ** 62)
        x[6::16] = 1
        return x
    if dt == np.float32:
        x = (rng.standard_normal(count) * 100).astype(np.float32)
        x[::5] = 0.0
        x[1::9] = -1.0
        return x
    x = rng.standard_normal(count) * 10.0 ** rng.integers(-20, 21, count)
    x[::5] = 0.0
    x[1::9] = -1.0
    x[2::9] = 1.0e20
    x[3::9] = -1.0e-20
    return x


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("name", ALL_KEYS)
def test_mul_vs_oracle(keys, name, dt):
    """Negative scalars in every call: k_inv_up / k_inv_down run at each group size (segments of 4)."""
    N = _native()
    ctx, key = keys(name)
    rng = np.random.default_rng(key.n.bit_length() + np.dtype(dt).num)
    nmax = max(MUL_N)
    cs = _rand_cts(rng, key, nmax)
    ex = rng.integers(-20, 41, nmax).astype(np.int32)
    x = _mul_scalars(rng, nmax, dt)
    assert (x < 0).sum() >= 10 and x[0] == 0
    want = [O.mul_scalar(cs[i], int(ex[i]), _py(x[i], dt), key) for i in range(nmax)]
    words = N.ints_to_words(cs, ctx.ct_words)
    for n in MUL_N:
        if n == 1:                                   # the scalar form (x_stride 0): a negative one, so the inversion runs
            xs, w = x[1:2], [want[1]]
            out, oe, st = ctx.mul(words[1:2], ex[1:2], xs)
        else:
            xs, w = x[:n], want[:n]
            out, oe, st = ctx.mul(words[:n], ex[:n], xs)
        assert np.all(st == 0)
        _same(out, oe, w, f"mul {name} {np.dtype(dt).name} N={n}")


# --------------------------------------------------------------------------- add_plain
@pytest.mark.parametrize("name", ALL_KEYS)
def test_add_plain_vs_oracle(keys, name):
    """The mix of test_gpu_add_plain.py::test_add_plain_vs_oracle_random (ciphertext exponents 0 .. 40) at every key.
    The elements the oracle refuses (x * 16^E beyond a double) are written out: they carry a status, all others
    compare equal."""
    N = _native()
    ctx, key = keys(name)
    count = 33
    rng = np.random.default_rng(key.n.bit_length() + 7)
    cs = _rand_cts(rng, key, count)
    ex = rng.integers(0, 41, count).astype(np.int32)
    words = N.ints_to_words(cs, ctx.ct_words)
    f64 = rng.standard_normal(count) * 10.0 ** rng.integers(-30, 30, count)
    f64[::5] = 0.0
    f64[1::7] = -1e-205
    f32 = (rng.standard_normal(count) * 1e3).astype(np.float32)
    i64 = rng.integers(-(2 ** 40), 2 ** 40, count, dtype=np.int64)
    i64[::4] = 0
    for x in (f64, f32, i64, np.array([-0.375]), np.array([9], dtype=np.int64)):
        out, oe, st = ctx.add_plain(words, ex, x)
        dt = x.dtype.type
        want = [O.add_scalar(cs[i], int(ex[i]), _py(x[i] if x.size == count else x[0], dt), key) for i in range(count)]
        assert np.all(st == 0), (name, x.dtype)      # |x| 16^40 stays far inside a double and inside n / 3 at 512 bits
        _same(out, oe, want, f"add_plain {name} {x.dtype}")


# --------------------------------------------------------------------------- matmul (term path), segment_add
@pytest.mark.parametrize("m,K,d", [(2, 5, 2), (1, 17, 1), (3, 33, 2)])
@pytest.mark.parametrize("name", ALL_KEYS)
def test_matmul_term_path_vs_oracle(keys, name, m, K, d):
    N = _native()
    ctx, key = keys(name)
    rng = np.random.default_rng(key.n.bit_length() + 100 * K + d)
    cs = _rand_cts(rng, key, m * K)
    ex = rng.integers(-6, 7, m * K).astype(np.int32)
    x = rng.standard_normal((K, d)) * 10.0 ** rng.integers(-3, 4, (K, d))
    x.flat[::5] = 0.0
    x.flat[1::3] = -np.abs(x.flat[1::3])
    x.flat[2::9] = -1.0
    assert (x < 0).any() and (x > 0).any()
    out, oe = ctx.matmul(N.ints_to_words(cs, ctx.ct_words), ex, m, K, x, d)
    assert ctx.matmul_path == 1
    want = []
    for i in range(m):
        for j in range(d):
            terms = [O.mul_scalar(cs[i * K + k], int(ex[i * K + k]), float(x[k, j]), key) for k in range(K)]
            want.append(O.add_k([t[0] for t in terms], [t[1] for t in terms], key))
    _same(out, oe, want, f"matmul {name} {(m, K, d)}")


@pytest.mark.parametrize("name", ["K1035", "K2071"])
def test_matmul_fused_path_at_the_seams(keys, xlib, monkeypatch, name):
    """The fused kernels (kernels_mm.hpp) and the k_add tree over their chunk partials where the ciphertext rows are no
    multiple of 4 words: the test build under $FLEXPAI_MM_ALWAYS=1 (tests/test_gpu_mm.py), two chunks of 16 and 1."""
    N = _native()
    _, key = keys(name)
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")
    ctx = N.Context(key.n, 0, lib=xlib)
    assert ctx.ct_words % 4 != 0
    m, K, d = 2, 17, 2
    rng = np.random.default_rng(key.n.bit_length() + 17)
    cs = _rand_cts(rng, key, m * K)
    ex = rng.integers(-6, 7, m * K).astype(np.int32)
    x = rng.standard_normal((K, d)) * 10.0 ** rng.integers(-3, 4, (K, d))
    x.flat[::5] = 0.0
    x.flat[1::3] = -np.abs(x.flat[1::3])
    out, oe = ctx.matmul(N.ints_to_words(cs, ctx.ct_words), ex, m, K, x, d)
    assert ctx.matmul_path == 2
    want = []
    for i in range(m):
        for j in range(d):
            terms = [O.mul_scalar(cs[i * K + k], int(ex[i * K + k]), float(x[k, j]), key) for k in range(K)]
            want.append(O.add_k([t[0] for t in terms], [t[1] for t in terms], key))
    _same(out, oe, want, f"fused matmul {name}")


@pytest.mark.parametrize("name", ALL_KEYS)
def test_segment_add_vs_oracle(keys, name):
    N = _native()
    ctx, key = keys(name)
    sizes = [0, 1, 2, 15, 16, 17, 257]
    M = 300
    rng = np.random.default_rng(key.n.bit_length() + 13)
    cs = _rand_cts(rng, key, M)
    ex = rng.integers(0, 21, M).astype(np.int32)
    members = [rng.integers(0, M, s) for s in sizes]
    idx = np.concatenate(members).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out, oe = ctx.segment_add(N.ints_to_words(cs, ctx.ct_words), ex, idx, off)
    want = [O.add_k([cs[i] for i in mem], [int(ex[i]) for i in mem], key) if len(mem) else (1, INT32_MIN)
            for mem in members]
    _same(out, oe, want, f"segment_add {name}")


# --------------------------------------------------------------------------- wide adds
def _wide_add(ctx, key, cs, ex, what):
    N = _native()
    k, n = ex.shape
    want = [O.add_k([cs[j][i] for j in range(k)], [int(ex[j, i]) for j in range(k)], key) for i in range(n)]
    out, oe = ctx.add([N.ints_to_words(c, ctx.ct_words) for c in cs], list(ex))
    _same(out, oe, want, what)


@pytest.mark.parametrize("k", [63, 64, 65, 129, 200])
def test_add_more_operands_than_one_launch(k1024, k):
    """k > 64 takes add_dev's split (kernels.hpp ADD_KMAX): 65 = 64 + 1, 129 = 64 + 64 + 1, 200 = 3 * 64 + 8, then
    a sum of the 2, 3, 4 partial sums. Exponents 0 .. 8, every fourth column all equal."""
    ctx, key = k1024
    n = 40
    rng = np.random.default_rng(k)
    cs = [_rand_cts(rng, key, n) for _ in range(k)]
    ex = rng.integers(0, 9, (k, n)).astype(np.int32)
    ex[:, ::4] = ex[0, ::4]
    _wide_add(ctx, key, cs, ex, f"add k={k}")


def test_add_65_operands_8_lanes(keys):
    ctx, key = keys("K4096")
    k, n = 65, 5
    rng = np.random.default_rng(65)
    cs = [_rand_cts(rng, key, n) for _ in range(k)]
    ex = rng.integers(0, 4, (k, n)).astype(np.int32)
    ex[:, 0] = 2
    _wide_add(ctx, key, cs, ex, "add K4096 k=65")


def test_add_montgomery_corrections_of_64_operands(k1024):
    """64 operands on one exponent level close with R^64; 63 on the lowest level and one above change level with R^64
    (kernels.hpp k_add: s = mcount at the end, s = 1 + mcount at a level change)."""
    ctx, key = k1024
    k, n = 64, 40
    rng = np.random.default_rng(64)
    cs = [_rand_cts(rng, key, n) for _ in range(k)]
    flat = np.repeat(rng.integers(-20, 41, (1, n)), k, axis=0).astype(np.int32)
    _wide_add(ctx, key, cs, flat, "add k=64, one level")
    step = flat.copy()
    for i in range(n):                               # the one higher operand at a different position in every column
        step[(7 * i + 3) % k, i] += 1 + i % 3
    _wide_add(ctx, key, cs, step, "add k=64, 63 + 1")


def test_add_schedule_bucket_clamp(k1024):
    """k = 33 with exponent gaps 0, 1, 255, 256 and 300 in one launch: 33, 38, 1054, 1058 and 1234 products
    (kernels.hpp add_steps: k - 1 + 4 gap + levels - 1 + 1), so k_add_plan clamps the last three to bucket
    ADD_TMAX - 1 = 1023 while the first sits in bucket 33. Every instance is checked."""
    ctx, key = k1024
    k, n = 33, 40
    gaps = [0, 1, 255, 256, 300]
    rng = np.random.default_rng(33)
    cs = [_rand_cts(rng, key, n) for _ in range(k)]
    ex = np.empty((k, n), dtype=np.int32)
    for i in range(n):
        base = int(rng.integers(-20, 21))
        low = rng.choice(k, size=3, replace=False)   # three operands on the low level, 30 on the high one
        ex[:, i] = base + gaps[i % len(gaps)]
        ex[low, i] = base
    assert sorted(set(int(g) for g in ex.max(axis=0) - ex.min(axis=0))) == gaps
    _wide_add(ctx, key, cs, ex, "add k=33, gaps to 300")


# --------------------------------------------------------------------------- batch inversion
def _sign_pattern(rng, n, long_runs):
    """+-1 in runs of irregular length: short runs of 1 .. 11, and runs of 70 and more so that whole segments (of up to
    64 values) hold no flagged element, and others only flagged ones."""
    x = np.empty(n, dtype=np.int64)
    pos, sign = 0, -1
    while pos < n:
        run = int(rng.choice([1, 1, 2, 3, 5, 7, 11, *long_runs]))
        x[pos:pos + run] = sign
        pos += run
        sign = -sign
    x[-1] = -1                                       # the ragged last segment inverts too
    return x


def _check_inversion(ctx, key, n, seed, long_runs=(70, 131, 200)):
    N = _native()
    rng = np.random.default_rng(seed)
    ct = rng.integers(0, 2 ** 32, (n, ctx.ct_words), dtype=np.uint32)
    ct[:, -1] = 0                                    # < 2^(32 (W - 1)) < n^2
    ex = rng.integers(-5, 6, n).astype(np.int32)
    x = _sign_pattern(rng, n, long_runs)
    neg = np.flatnonzero(x < 0)
    pos = np.flatnonzero(x > 0)
    assert min(len(neg), len(pos)) >= n // 5
    runs = np.diff(np.flatnonzero(np.diff(x)))           # lengths of the inner runs
    assert runs.max() >= 70 and len(set(runs.tolist())) >= 5
    out, oe, st = ctx.mul(ct, ex, x)
    assert np.array_equal(oe, ex) and not st.any()
    assert np.array_equal(out[pos], ct[pos]), "c * 1 changed"
    a = N.words_to_ints(np.ascontiguousarray(out[neg]))
    b = N.words_to_ints(np.ascontiguousarray(ct[neg]))
    n2 = key.nsquare
    bad = [int(neg[i]) for i in range(len(neg)) if a[i] >= n2 or a[i] * b[i] % n2 != 1]
    assert not bad, f"{len(bad)} of {len(neg)} inverses wrong, first at {bad[:8]}"


@pytest.mark.parametrize("n,seg_len", [(20483, 5), (69633, 17), (262181, 64)])
def test_batch_inversion_segment_lengths(k1024, n, seg_len):
    """mul by -1 / +1 over n values: the first inversion level runs segments of 5, 17 and 64 values (flexpai.hip
    batch_invert: max(4, min(INV_SEG, n / 4096)); 262144 is the smallest n with full segments), each n with a ragged
    last segment. Every element is checked: out * c == 1 mod n^2 for -1, out == c for +1."""
    ctx, key = k1024
    assert max(4, min(64, n // 4096)) == seg_len and n % seg_len != 0
    _check_inversion(ctx, key, n, n)


def test_batch_inversion_8_lanes(keys):
    """300 values at 4096 bits: three levels of segments of 4 on k_inv_up<8> / k_inv_down<8>."""
    ctx, key = keys("K4096")
    _check_inversion(ctx, key, 300, 4101, long_runs=(70,))


# --------------------------------------------------------------------------- k_plain: the shifted multiplier
BIG = 2 ** 62 + 12345


def _shift_starts(nb, lanes):
    """Limbs q at which the multiplier's four digits start: the first, a middle and the last limb of every lane, and the
    three starts that straddle each lane seam; kept where a one-bit multiplier at that limb is inside the range check
    (|M| <= nb - 3 bits: lanes past nb / 28 limbs cannot be reached by a valid encoding)."""
    qs = set()
    for t in range(lanes):
        qs |= {LANE_LIMBS * t, LANE_LIMBS * t + 18, LANE_LIMBS * t + 36}
        if t:
            qs |= {LANE_LIMBS * t - 1, LANE_LIMBS * t - 2, LANE_LIMBS * t - 3}
    qmax = (nb - 4) // LIMB_BITS
    return sorted(q for q in qs | {qmax} if q <= qmax)


@pytest.mark.parametrize("name", ["K2071", "K4096"])
def test_add_plain_shift_across_lanes(keys, name):
    """int64 scalars on ciphertext exponent E: |M| = |x| 16^E exactly, sh = 4 E, so E = 7 q + r puts the digits at limb
    q with sh mod 28 = 4 r. Ciphertexts alternate between the value 1 (the sum is k_plain's own 1 + n M) and random
    units. All of these are inside the range check: status 0, equal to the oracle."""
    N = _native()
    ctx, key = keys(name)
    nb = key.n.bit_length()
    starts = _shift_starts(nb, LANES[name])
    assert starts[-1] // LANE_LIMBS >= LANES[name] // 2 - 1 and len(starts) >= 3 * LANES[name] // 2
    es, xs = [], []
    for q in starts:
        for r in (0, 1, 6):
            E = 7 * q + r
            for x in (1, -1, 0, BIG, -BIG):
                if abs(x).bit_length() + 4 * E <= nb - 3:
                    es.append(E)
                    xs.append(x)
    seen = {(E // 7, x) for E, x in zip(es, xs)}
    assert all((q, 1) in seen and (q, -1) in seen for q in starts)
    assert all((q, BIG) in seen and (q, -BIG) in seen for q in starts if q <= starts[-1] - 3)
    rng = np.random.default_rng(nb)
    units = _rand_cts(rng, key, len(es))
    cs = [1 if i % 2 == 0 else units[i] for i in range(len(es))]
    ex = np.array(es, dtype=np.int32)
    out, oe, st = ctx.add_plain(N.ints_to_words(cs, ctx.ct_words), ex, np.array(xs, dtype=np.int64))
    assert not st.any()
    want = [O.add_scalar(c, E, x, key) for c, E, x in zip(cs, es, xs)]
    _same(out, oe, want, f"add_plain {name} shifts")


@pytest.mark.parametrize("name", ["K2071", "K4096"])
def test_add_plain_float_shifts_and_overflow(keys, name):
    """float64 scalars on exponents up to 255: sh = fe - 53 + 4 E (up to 971 bits). The two written-out cases, E >= 256
    and fe + 4 E > 1024, are OverflowError in the oracle and PAI_EL_FLOAT_OVF on the device."""
    N = _native()
    ctx, key = keys(name)
    cases = [(E, v) for E in (41, 100, 101, 199, 254, 255) for v in (1.0, -1.5, 0.1, -7.25e-3, 0.0, 15.999999999999998)]
    cases += [(249, 2.0 ** 24 * 1.0000000000000002), (255, 8.0 - 2.0 ** -50), (255, -2.0 ** -60)]
    overflow = [(256, 1.0), (255, 1024.0)]
    for E, v in overflow:
        with pytest.raises(OverflowError):
            O.add_scalar(1, E, v, key)
    allc = cases + overflow
    rng = np.random.default_rng(key.n.bit_length() + 1)
    units = _rand_cts(rng, key, len(allc))
    cs = [1 if i % 2 == 0 else units[i] for i in range(len(allc))]
    ex = np.array([E for E, _ in allc], dtype=np.int32)
    out, oe, st = ctx.add_plain(N.ints_to_words(cs, ctx.ct_words), ex, np.array([v for _, v in allc]))
    assert list(st[len(cases):]) == [N.EL_FLOAT_OVF] * len(overflow)
    assert not st[:len(cases)].any()
    want = [O.add_scalar(c, E, v, key) for c, (E, v) in zip(cs, cases)]
    _same(out[:len(cases)], oe[:len(cases)], want, f"add_plain {name} float shifts")


@pytest.mark.parametrize("name", ALL_KEYS)
def test_add_plain_range_boundary(keys, name):
    """|M| of exactly nb - 3 bits is encoded (status 0, the oracle's bits: 2^(nb - 3) < n / 3); |M| of nb - 2 bits is
    PAI_EL_ENC_RANGE (include/flexpai.h: the exact |M| > max_int test is the caller's), and so is a multiplier a
    million hex digits past the range (exponent 2^20, far beyond the group's limbs)."""
    N = _native()
    ctx, key = keys(name)
    nb = key.n.bit_length()
    b = (nb - 3) % 4 or 4
    E = (nb - 3 - b) // 4
    inside = [(1 << b) - 1, -((1 << (b - 1)) | 1 if b > 1 else 1)]
    outside = [1 << b, -((1 << (b + 1)) - 1)]
    far = [1, -BIG]
    xs = inside + outside + far
    assert all(abs(x).bit_length() + 4 * E == nb - 3 for x in inside)
    assert all(abs(x).bit_length() + 4 * E == nb - 2 for x in outside)
    rng = np.random.default_rng(nb + 3)
    cs = [1, _rand_cts(rng, key, 1)[0], 1, 1, 1, 1]
    ex = np.array([E] * 4 + [1 << 20] * 2, dtype=np.int32)
    out, oe, st = ctx.add_plain(N.ints_to_words(cs, ctx.ct_words), ex, np.array(xs, dtype=np.int64))
    assert list(st) == [0, 0] + [N.EL_ENC_RANGE] * 4
    want = [O.add_scalar(c, E, x, key) for c, x in zip(cs[:2], inside)]
    _same(out[:2], oe[:2], want, f"add_plain {name} at nb - 3 bits")
