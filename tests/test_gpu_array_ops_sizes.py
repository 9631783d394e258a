"""GPU parity of the array operators (fused pai_matmul, pai_segment_dot, pai_histogram, pai_histogram_sparse, pai_cumsum,
pai_obfuscate, pai_encrypt_packed / pai_decrypt_packed, pai_pack_ciphertexts, pai_check_below_dev, pai_take_dev) against
the oracle on Python integers, bit for bit and on every output, at the lane-group seams and at top-heavy moduli:

  K512, K1035, K1036, K2071, K2072, K3072   the seeded keys of tests/test_gpu_ops_sizes.py: groups of 2, 2, 4, 4, 8, 8
                                            lanes; ct_words 65 and 130 (no multiple of 4) at 1035 and 2071 bits
  K1035T   p = 2^518 - 917, q = 2^517 - 489       the largest primes below 2^518 and 2^517
  K2071T   p = 2^1036 - 1127, q = 2^1035 - 441    the largest primes below 2^1036 and 2^1035

At 1035 and 2071 bits 2 nb + 2 fills the group's 28 * 37 * TPI limb bits exactly, so R = 2^(2 nb + 2) is the smallest
Montgomery radix the lazy reduction allows (R >= 4 n^2, bn_group.hpp montmul). The seeded keys put n^2 / R at a random
fraction of 1/4; the top-heavy ones put 4 n^2 within R / 2^500 of R, where a chain of unreduced products (window
tables, squarings, a Horner fold, a scan) has no slack left (test_top_heavy_preconditions asserts all of this). On the
top-heavy keys the operands also hold the residues that make the intermediates large: n^2 - 1, n^2 - 2, n + 1,
(n^2 -+ 1) / 2 and 1, as the first and the last operand of a chain and as a multiplier's base (_operands).

The oracle (oracle/paillier_oracle.py) does not depend on the key size and is pinned by the golden tests. The expected
values reuse the helpers of the per-operator modules (test_gpu_mm._oracle_dot, test_gpu_packed.expected_c0 / unpack,
test_gpu_hist.lists_from_bins). Keys, contexts and r^n mod n^2 per (key, r) are made once per module."""
import math

import numpy as np
import pytest

from oracle import paillier_oracle as O
from test_gpu_hist import lists_from_bins
from test_gpu_mm import _oracle_dot, _scalars
from test_gpu_ops_sizes import GENERATED, LANE_LIMBS, LIMB_BITS, _make_key, _rand_cts, _same
from test_gpu_packed import _patterns, expected_c0, unpack, values_from_t

pytestmark = pytest.mark.gpu
EMPTY = -(1 << 31)
SEEDED = ["K512", "K1035", "K1036", "K2071", "K2072", "K3072"]
TKEYS = ["K1035T", "K2071T"]
KEYS = SEEDED + TKEYS
BITS = {"K512": 512, "K1035T": 1035, "K2071T": 2071, **{k: v[0] for k, v in GENERATED.items()}}
LANES = {"K512": 2, "K1035T": 2, "K2071T": 4, **{k: v[4] for k, v in GENERATED.items()}}
T_PRIMES = {"K1035T": ((1 << 518) - 917, (1 << 517) - 489), "K2071T": ((1 << 1036) - 1127, (1 << 1035) - 441)}
HIST_ENV = ("FLEXPAI_HIST_ACC", "FLEXPAI_HIST_RUN", "FLEXPAI_HIST_SCRATCH_BYTES", "FLEXPAI_HIST_CHUNK")


def _native():
    from flex.crypto.paillier import _native
    return _native


class _Keys:
    """Keys, contexts (public on the product library, public on the test build, key holder) and the oracle's r^n mod
    n^2 per (key, r): made on first use and kept for the module."""

    def __init__(self, golden, xlib):
        self.golden, self.xlib, self.keys, self.ctxs, self.rn = golden, xlib, {}, {}, {}

    def key(self, name):
        if name not in self.keys:
            self.keys[name] = _make_key(name, self.golden)
            assert self.keys[name].n.bit_length() == BITS[name]
        return self.keys[name]

    def _ctx(self, name, kind):
        if (name, kind) not in self.ctxs:
            key, N = self.key(name), _native()
            self.ctxs[name, kind] = (N.Context(key.n, 0, key.p, key.q) if kind == "holder" else
                                     N.Context(key.n, 0, lib=self.xlib) if kind == "xpublic" else N.Context(key.n, 0))
        return self.ctxs[name, kind], self.key(name)

    def public(self, name):
        return self._ctx(name, "public")

    def xpublic(self, name):
        """On the test build: it reads $FLEXPAI_MM_ALWAYS, $FLEXPAI_SD_ALWAYS and $FLEXPAI_HIST_ACC at every call."""
        return self._ctx(name, "xpublic")

    def holder(self, name):
        return self._ctx(name, "holder")

    def r_pow_n(self, key, r):
        if (key.n, r) not in self.rn:
            self.rn[key.n, r] = pow(r, key.n, key.nsquare)
        return self.rn[key.n, r]


@pytest.fixture(scope="module")
def K(golden, xlib):
    return _Keys(golden, xlib)


def _extremes(key):
    """The residues that make unreduced intermediates large; all of them units mod n^2."""
    n2 = key.nsquare
    return [n2 - 1, key.n + 1, (n2 - 1) // 2, 1, (n2 + 1) // 2, n2 - 2]


def _operands(name, key, count, seed):
    """`count` random ciphertexts below n^2. On the top-heavy keys the first three and the last three are the extreme
    residues: every case lays its chains out so that element 0 opens one and element count - 1 closes one."""
    cs = _rand_cts(np.random.default_rng(seed), key, count)
    if name in TKEYS:
        assert count >= 6
        x = _extremes(key)
        cs[:3], cs[-3:] = x[:3], x[3:]
    return cs


def _words(ctx, cs):
    return _native().ints_to_words(list(cs), ctx.ct_words)


# --------------------------------------------------------------------------- the keys
@pytest.mark.parametrize("name", TKEYS)
def test_top_heavy_preconditions(K, name):
    """What makes these keys the edge: a later change to the construction or to the engine's sizing fails here."""
    ctx, key = K.public(name)
    nb, tpi = BITS[name], LANES[name]
    assert (key.q, key.p) == T_PRIMES[name] and all(O._is_probable_prime(h) for h in (key.p, key.q))
    assert key.n.bit_length() == nb == ctx.key_bits
    assert 2 * nb + 2 == LIMB_BITS * LANE_LIMBS * tpi
    R = 1 << (LIMB_BITS * LANE_LIMBS * tpi)
    assert 4 * key.nsquare < R and R - 4 * key.nsquare < R >> 500
    assert (1 << 2 * nb) - key.nsquare < 1 << (2 * nb - 500)
    assert ctx.ct_words == (2 * nb + 31) // 32 and ctx.ct_words % 4 != 0
    assert ctx.pt_words == (nb + 31) // 32 and nb % 32 != 0
    assert all(math.gcd(c, key.n) == 1 for c in _extremes(key))
    # the key holder's routes above the rows: the lane CRT and the pair kernels at 1035 bits (q mod (p - 1) = 63 there:
    # setup_crt's stage_a_exponent), the group engine alone at 2071
    holder, _ = K.holder(name)
    assert holder.crt_available == holder.lane_decrypt == (name == "K1035T")
    assert holder.pair_paths & 1 == (name == "K1035T")


@pytest.mark.parametrize("name", SEEDED)
def test_seeded_key_shapes(K, name):
    ctx, key = K.public(name)
    nb = BITS[name]
    assert ctx.key_bits == nb and ctx.ct_words == (2 * nb + 31) // 32 and ctx.pt_words == (nb + 31) // 32
    assert next(t for t in (2, 4, 8) if LIMB_BITS * LANE_LIMBS * t >= 2 * nb + 2) == LANES[name]


# --------------------------------------------------------------------------- 1. fused matrix product
@pytest.mark.parametrize("dt", [np.float64, np.int64])
@pytest.mark.parametrize("name", KEYS)
def test_matmul_fused(K, monkeypatch, name, dt):
    """m = 2, K = 17 (one chunk of MM_KC = 16 plus one), d = 3; zeros, -0.0, -1.0 and +-2^62 among the scalars, so the
    inverse tables and the 16-window exponents run. Exponents -6 .. 6: D > 0 inside both chunks."""
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")
    ctx, key = K.xpublic(name)
    m, Kk, d = 2, 17, 3
    cs = _operands(name, key, m * Kk, BITS[name] + 1)
    es = [int(e) for e in np.random.default_rng(BITS[name]).integers(-6, 7, m * Kk)]
    x = _scalars(Kk, d, dt, 3 * Kk + d)
    assert (x < 0).any() and (x == 0).any() and len(set(es[:16])) > 1
    out, oe = ctx.matmul(_words(ctx, cs), np.array(es, dtype=np.int32), m, Kk, x, d)
    assert ctx.matmul_path == 2
    _same(out, oe, _oracle_dot(cs, es, m, Kk, x, d, key), f"fused matmul {name} {np.dtype(dt).name}")


@pytest.mark.parametrize("name", TKEYS)
def test_matmul_fused_longest_chain(K, monkeypatch, name):
    """One chunk of 16 extreme residues, every scalar 2^62 - 1: 16 windows of all-ones digits (the table's top power at
    every window) and four squarings between them, over the largest residues."""
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")
    ctx, key = K.xpublic(name)
    ext = _extremes(key)
    cs = [ext[i % len(ext)] for i in range(16)]
    cs[15] = ext[5]
    for es in ([0] * 16, [i % 3 for i in range(16)]):
        x = np.full((16, 1), 2 ** 62 - 1, dtype=np.int64)
        out, oe = ctx.matmul(_words(ctx, cs), np.array(es, dtype=np.int32), 1, 16, x, 1)
        assert ctx.matmul_path == 2
        _same(out, oe, _oracle_dot(cs, es, 1, 16, x, 1, key), f"fused matmul {name}, extreme residues")


def _non_units(key):
    return [key.n, key.p * key.n]


@pytest.mark.parametrize("name", KEYS)
def test_matmul_fused_not_invertible(K, monkeypatch, name):
    """n and p n share a factor with n: the oracle's bits under positive scalars and under a negative scalar in another
    row of x, ZeroDivisionError (PAI_ERR_NOINV) once their own row holds one (test_gpu_mm.py::test_not_invertible)."""
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")
    ctx, key = K.xpublic(name)
    cs = _operands(name, key, 6, BITS[name] + 2)
    cs[2:4] = _non_units(key)
    es = [3, 0, 2, 5, 1, 4]
    ct, ex = _words(ctx, cs), np.array(es, dtype=np.int32)
    x = np.array([[1.0, 2.0], [0.5, 3.0], [2.0, 7.0], [4.0, 1.0], [5.0, 6.0], [0.25, 9.0]])
    for neg_row in (None, 4):
        xs = x.copy()
        if neg_row is not None:
            xs[neg_row, 1] = -xs[neg_row, 1]
        out, oe = ctx.matmul(ct, ex, 1, 6, xs, 2)
        assert ctx.matmul_path == 2
        _same(out, oe, _oracle_dot(cs, es, 1, 6, xs, 2, key), f"fused matmul {name}, non-units, negative row {neg_row}")
    for row in (2, 3):
        xs = x.copy()
        xs[row, 0] = -2.0
        with pytest.raises(ZeroDivisionError):
            ctx.matmul(ct, ex, 1, 6, xs, 2)


# --------------------------------------------------------------------------- 2. segment_dot
SD_LENS = (7, 0, 16, 1, 9, 7)           # 40 entries: a full chunk of 16, an empty segment, ragged ones
SD_NCT = 9


def _sd_case(seed):
    rng = np.random.default_rng(seed)
    nnz = sum(SD_LENS)
    off = np.concatenate([[0], np.cumsum(SD_LENS)]).astype(np.int64)
    idx = rng.integers(0, SD_NCT, nnz).astype(np.int64)
    idx[0], idx[-1] = 0, SD_NCT - 1                     # the first and the last operand of a chain
    idx[7:7 + SD_NCT] = np.arange(SD_NCT)               # every ciphertext inside the 16-entry chunk: its table is shared
    x = (np.abs(rng.standard_normal(nnz)) + 0.1) * 10.0 ** rng.integers(-6, 7, nnz)
    x = np.where(rng.random(nnz) < 0.4, -x, x)
    x[0], x[-1], x[12] = -abs(x[0]), abs(x[-1]), 0.0
    return idx, off, x


def _sd_run(ctx, fused, *args):
    ctx.set_segdot_fused(fused)
    try:
        res = ctx.segment_dot(*args)
        assert ctx.segdot_path == (2 if fused else 1)
    finally:
        ctx.set_segdot_fused(True)
    return res


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", KEYS)
def test_segment_dot(K, monkeypatch, name, fused):
    """The fused kernels (k_sd_acc over k_mm_tab's tables, forced by $FLEXPAI_SD_ALWAYS on the test build) and the gather
    + k_mul path: O.mul_scalar per entry, O.add_k per segment."""
    monkeypatch.setenv("FLEXPAI_SD_ALWAYS", "1")
    for k in ("FLEXPAI_MM_TABLE_BYTES", "FLEXPAI_SD_SLICE"):
        monkeypatch.delenv(k, raising=False)
    ctx, key = K.xpublic(name)
    cs = _operands(name, key, SD_NCT, BITS[name] + 3)
    es = [int(e) for e in np.random.default_rng(BITS[name] + 3).integers(0, 21, SD_NCT)]
    idx, off, x = _sd_case(BITS[name])
    assert (x < 0).sum() >= 8 and np.unique(idx).size == SD_NCT
    want = []
    for a, b in zip(off[:-1], off[1:]):
        terms = [O.mul_scalar(cs[idx[t]], es[idx[t]], float(x[t]), key) for t in range(a, b)]
        want.append(O.add_k([t[0] for t in terms], [t[1] for t in terms], key) if terms else (1, EMPTY))
    out, oe, st = _sd_run(ctx, fused, _words(ctx, cs), np.array(es, dtype=np.int32), idx, off, x)
    assert not st.any()
    _same(out, oe, want, f"segment_dot {name} fused={fused}")


@pytest.mark.parametrize("name", KEYS)
def test_segment_dot_not_invertible(K, monkeypatch, name):
    """test_gpu_segdot.py::test_errors at this key, with n and p n: fine under positive scalars, no inverse under a
    negative one, on both paths."""
    monkeypatch.setenv("FLEXPAI_SD_ALWAYS", "1")
    ctx, key = K.xpublic(name)
    cs = _operands(name, key, 6, BITS[name] + 4)[:4] + _non_units(key)
    es = [2, 0, 1, 3, 1, 0]
    ct, ex = _words(ctx, cs), np.array(es, dtype=np.int32)
    idx, off = np.array([0, 4, 2, 5, 1], dtype=np.int64), np.array([0, 2, 5], dtype=np.int64)
    for fused in (True, False):
        x = np.array([1.0, 2.0, -3.0, 4.0, -0.5])
        want = []
        for a, b in zip(off[:-1], off[1:]):
            terms = [O.mul_scalar(cs[idx[t]], es[idx[t]], float(x[t]), key) for t in range(a, b)]
            want.append(O.add_k([t[0] for t in terms], [t[1] for t in terms], key))
        out, oe, st = _sd_run(ctx, fused, ct, ex, idx, off, x)
        assert not st.any()
        _same(out, oe, want, f"segment_dot {name}, non-units, fused={fused}")
        for x in (np.array([1.0, -2.0, 3.0, 4.0, 0.5]), np.array([1.0, 2.0, 3.0, -4.0, 0.5])):
            ctx.set_segdot_fused(fused)
            try:
                with pytest.raises(ZeroDivisionError):
                    ctx.segment_dot(ct, ex, idx, off, x)
            finally:
                ctx.set_segdot_fused(True)


# --------------------------------------------------------------------------- 3, 4. histograms
H_N, H_F, H_B, H_NODES = 70, 2, 3, 2
H_DEFAULT = np.array([0, 1], dtype=np.int32)


def _hist_case(seed):
    """(bins [70, 2] with ids 0 .. 3, 3 = B is in no cell; node ids 0 / 1). Sample 0 opens a cell and sample 69 closes
    one in both features."""
    rng = np.random.default_rng(seed)
    bins = rng.integers(0, H_B + 1, (H_N, H_F))
    bins[0], bins[-1] = (0, 2), (2, 1)
    node = rng.integers(0, H_NODES, H_N).astype(np.int32)
    assert (bins == H_B).sum() >= 10
    return bins, node


def _hist_want(cs, es, bins, node, key):
    idx, off = lists_from_bins(bins, H_B, node, H_NODES)
    want = []
    for a, b in zip(off[:-1], off[1:]):
        mem = idx[a:b].tolist()
        want.append(O.add_k([cs[i] for i in mem], [es[i] for i in mem], key) if mem else (1, EMPTY))
    return want, np.diff(off)


@pytest.mark.parametrize("dtype,acc", [(np.uint8, None), (np.uint16, None), (np.uint8, "0")],
                         ids=["u8", "u16", "u8-rows"])
@pytest.mark.parametrize("name", KEYS)
def test_histogram(K, monkeypatch, name, dtype, acc):
    """k_hist_acc over the runs (the default) and, under $FLEXPAI_HIST_ACC=0 on the test build, k_hist_rows + k_add."""
    for k in HIST_ENV:
        monkeypatch.delenv(k, raising=False)
    if acc is not None:
        monkeypatch.setenv("FLEXPAI_HIST_ACC", acc)
    ctx, key = K.xpublic(name)
    cs = _operands(name, key, H_N, BITS[name] + 5)
    es = [int(e) for e in np.random.default_rng(BITS[name] + 5).integers(0, 21, H_N)]
    bins, node = _hist_case(BITS[name])
    want, counts = _hist_want(cs, es, bins, node, key)
    out, oe, cnt = ctx.histogram(_words(ctx, cs), np.array(es, dtype=np.int32), bins.astype(dtype), H_B, node, H_NODES)
    assert np.array_equal(cnt, counts) and counts.min() >= 2
    _same(out, oe, want, f"histogram {name} {np.dtype(dtype).name} acc={acc}")


def _csr(bins):
    """The dense matrix as CSR: every entry off its feature's default bin is stored, the missing ids (B) included."""
    indptr, indices, data = [0], [], []
    for row in bins:
        for f in range(H_F):
            if row[f] != H_DEFAULT[f]:
                indices.append(f)
                data.append(row[f])
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data, dtype=np.uint8)


def _shist_want(cs, es, bins, node, key):
    """Cells off the default bin: O.add_k. The default cell: T S^-1 mod n^2 with T the node's sum, S the sum of the
    node's stored entries of the feature, aligned to T's exponent (include/flexpai.h)."""
    want, counts = _hist_want(cs, es, bins, node, key)
    n2 = key.nsquare
    for v in range(H_NODES):
        members = np.flatnonzero(node == v).tolist()
        T, te = O.add_k([cs[i] for i in members], [es[i] for i in members], key)
        for f in range(H_F):
            s = (v * H_F + f) * H_B + int(H_DEFAULT[f])
            rest = [i for i in members if bins[i, f] != H_DEFAULT[f]]
            assert rest and counts[s] == len(members) - len(rest) > 0
            S, se = O.add_k([cs[i] for i in rest], [es[i] for i in rest], key)
            want[s] = (T * pow(pow(S, -1, n2), 16 ** (te - se), n2) % n2, te)
    return want, counts


@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed"])
@pytest.mark.parametrize("name", KEYS)
def test_histogram_sparse(K, monkeypatch, name, mixed):
    for k in HIST_ENV:
        monkeypatch.delenv(k, raising=False)
    ctx, key = K.public(name)
    cs = _operands(name, key, H_N, BITS[name] + 6)
    es = [int(e) for e in np.random.default_rng(BITS[name] + 6).integers(0, 6, H_N)] if mixed else [3] * H_N
    bins, node = _hist_case(BITS[name] + 1)
    want, counts = _shist_want(cs, es, bins, node, key)
    if not mixed:                                            # uniform exponents: T S^-1 is the dense cell's own sum
        assert want == _hist_want(cs, es, bins, node, key)[0]
    out, oe, cnt = ctx.histogram_sparse(_words(ctx, cs), np.array(es, dtype=np.int32), *_csr(bins), H_F, H_DEFAULT, H_B,
                                        node, H_NODES)
    assert np.array_equal(cnt, counts)
    _same(out, oe, want, f"histogram_sparse {name} mixed={mixed}")


@pytest.mark.parametrize("name", ["K1035", "K2071", "K2072"])
def test_histogram_sparse_not_invertible(K, name):
    """n among the stored entries of feature 0: S has no inverse mod n^2 and the call ends with PAI_ERR_NOINV; with the
    sample's entry on the default bin (not stored) the same ciphertexts give the oracle's bits."""
    ctx, key = K.public(name)
    cs = _operands(name, key, H_N, BITS[name] + 7)
    es = [2] * H_N
    bins, node = _hist_case(BITS[name] + 2)
    cs[5] = key.n
    bins[5] = (1, 2)
    args = (_words(ctx, cs), np.array(es, dtype=np.int32))
    with pytest.raises(ZeroDivisionError):
        ctx.histogram_sparse(*args, *_csr(bins), H_F, H_DEFAULT, H_B, node, H_NODES)
    bins[5, 0] = H_DEFAULT[0]                                # now only feature 1 stores it, and inverts it
    with pytest.raises(ZeroDivisionError):
        ctx.histogram_sparse(*args, *_csr(bins), H_F, H_DEFAULT, H_B, node, H_NODES)
    bins[5, 1] = H_DEFAULT[1]                                # stored nowhere: no S holds it
    out, oe, cnt = ctx.histogram_sparse(*args, *_csr(bins), H_F, H_DEFAULT, H_B, node, H_NODES)
    want, counts = _hist_want(cs, es, bins, node, key)       # uniform exponents: T S^-1 = the dense sum, n a factor
    assert np.array_equal(cnt, counts)
    _same(out, oe, want, f"histogram_sparse {name}, n on the default bins")


# --------------------------------------------------------------------------- 5. cumsum
def _scan_want(cs, es, outer, L, inner, rev, key):
    """The O.add_k chain along the middle axis, in array order."""
    res = [None] * (outer * L * inner)
    for o in range(outer):
        for i in range(inner):
            acc = None
            for j in (range(L - 1, -1, -1) if rev else range(L)):
                t = (o * L + j) * inner + i
                acc = (cs[t], es[t]) if acc is None else O.add_k([acc[0], cs[t]], [acc[1], es[t]], key)
                res[t] = acc
    return res


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("name", KEYS)
def test_cumsum(K, name, rev):
    """(2, 70, 2): the automatic choice, the row chain (one tile holds the row) and the tiled scan with tiles of 32, 32
    and 6 (k_scan over the tiles, the scan of the tile totals, the fix-up)."""
    ctx, key = K.public(name)
    outer, L, inner = 2, 70, 2
    cs = _operands(name, key, outer * L * inner, BITS[name] + 8)
    es = [int(e) for e in np.random.default_rng(BITS[name] + 8).integers(0, 6, len(cs))]
    want = _scan_want(cs, es, outer, L, inner, rev, key)
    ct, ex = _words(ctx, cs), np.array(es, dtype=np.int32)
    try:
        for tile, path in ((0, None), (128, 1), (32, 2)):
            ctx.set_scan_tile(tile)
            out, oe = ctx.cumsum(ct, ex, outer, L, inner, reverse=rev)
            assert path is None or ctx.scan_path == path
            _same(out, oe, want, f"cumsum {name} rev={rev} tile={tile}")
    finally:
        ctx.set_scan_tile(0)


@pytest.mark.parametrize("name", TKEYS)
def test_cumsum_of_the_largest_residue(K, name):
    """70 copies of n^2 - 1 = -1 on one exponent: the prefixes alternate between n^2 - 1 and 1."""
    ctx, key = K.public(name)
    cs, es = [key.nsquare - 1] * 70, [4] * 70
    want = [(key.nsquare - 1 if j % 2 == 0 else 1, 4) for j in range(70)]
    assert want == _scan_want(cs, es, 1, 70, 1, False, key)
    try:
        for tile, path in ((128, 1), (32, 2)):
            ctx.set_scan_tile(tile)
            out, oe = ctx.cumsum(_words(ctx, cs), np.array(es, dtype=np.int32), 1, 70, 1)
            assert ctx.scan_path == path
            _same(out, oe, want, f"cumsum {name} of n^2 - 1, tile={tile}")
    finally:
        ctx.set_scan_tile(0)


# --------------------------------------------------------------------------- 6. obfuscate
def _obf_rs(key):
    """Explicit obfuscators, fewer at the larger keys (a 3072-bit pow takes 0.3 s): n - 1 and 2 stay."""
    nb = key.n.bit_length()
    seeded = 4 if nb <= 1100 else 2 if nb <= 2100 else 0
    return [key.n - 1, 2] + [O.golden_r(key.n, 4711, i) for i in range(seeded)]


@pytest.mark.parametrize("party", ["public", "holder"])
@pytest.mark.parametrize("name", KEYS)
def test_obfuscate_given_r(K, name, party):
    """k_obf_mul over the r^n of the explicit-r encrypt chain: c r^n mod n^2, for 1 and 65 ciphertexts."""
    N = _native()
    ctx, key = K.public(name) if party == "public" else K.holder(name)
    cs = _operands(name, key, 65, BITS[name] + 9)
    base = _obf_rs(key)
    rs = [base[i % len(base)] for i in range(65)]
    want = [c * K.r_pow_n(key, r) % key.nsquare for c, r in zip(cs, rs)]
    assert want[1] == cs[1] * pow(2, key.n, key.nsquare) % key.nsquare
    ct = _words(ctx, cs)
    for count in (1, 65):
        out = ctx.obfuscate(ct[:count], obf_mode=N.PAI_OBF_GIVEN, r=rs[:count])
        got = N.words_to_ints(out)
        bad = [i for i in range(count) if got[i] != want[i]]
        assert not bad, f"obfuscate {name} {party} N={count}: outputs differ from c r^n mod n^2 at {bad[:8]}"


# --------------------------------------------------------------------------- 7, 8. packed encrypt and decrypt
PACK_LAYOUTS = [pytest.param(16, 16, 3, np.float32, id="16-16-f32"), pytest.param(64, 64, 0, np.int64, id="64-64-i64")]
PACK_C = 65


def _pack_case(ctx, key, sb, vb, e, dtype):
    nb = key.n.bit_length()
    k = ctx.pack_max_slots(sb)
    assert k == (nb - 2) // sb
    lay = (sb, vb, e, k)
    ts = _patterns(PACK_C, k, vb, 1, nb + sb)
    x = values_from_t(ts, dtype, e)
    want, st_want, _ = expected_c0(x, lay, key.n)
    assert not any(st_want) and want[3] == 1
    # the all -mx row: M < 0, c0 = n^2 + 1 - n |M| with |M| of k sb - 1 bits, in the top limb of n
    assert want[1] == key.nsquare + 1 - key.n * sum(((1 << (vb - 1)) - 1) << (sb * j) for j in range(k))
    return lay, ts, x, want


@pytest.mark.parametrize("sb,vb,e,dtype", PACK_LAYOUTS)
@pytest.mark.parametrize("name", KEYS)
def test_encrypt_packed_c0(K, name, sb, vb, e, dtype):
    """k_pack_mul without an obfuscator: c0 = 1 + n (M mod n) for 1 and 65 ciphertexts over the six patterns."""
    N = _native()
    ctx, key = K.public(name)
    lay, ts, x, want = _pack_case(ctx, key, sb, vb, e, dtype)
    k = lay[3]
    for C in (1, PACK_C):
        ct, st = ctx.encrypt_packed(x[:C * k], lay, obf_mode=N.PAI_OBF_NONE)
        assert not st.any()
        got = N.words_to_ints(ct)
        bad = [i for i in range(C) if got[i] != want[i]]
        assert not bad, f"encrypt_packed {name} {lay} C={C}: c0 differs at {bad[:8]}"


@pytest.mark.parametrize("sb,vb,e,dtype", PACK_LAYOUTS)
@pytest.mark.parametrize("name", KEYS)
def test_decrypt_packed(K, name, sb, vb, e, dtype):
    """k_unpack behind the key holder's decrypt routes: on the rows, and with PAI_OPT_ROWS_MAX = 0 on the route above
    them (the pair kernels, k_dec4_*, or the group engine alone at 2071 bits). Values, mantissas and statuses follow
    `unpack`; then the sign test's boundaries.

    A plaintext in the gap between max_int and n - max_int reports overflow for every value of its ciphertext. So do
    m = max_int and m = n - max_int: they pass the sign test, but no legal layout holds them (k sb <= nb - 2, and
    max_int = n / 3 - 1 >= 2^(nb - 1) / 3 - 1 has at least nb - 2 bits, beyond the k sb - 1 bits of a signed M), which
    `unpack` states as its last line and k_unpack as the bits at and above B^k. The largest plaintexts a layout does
    hold, +-(2^(k sb - 1) - 1) from the all +-mx rows at vb = sb, decode on both sides of the sign test."""
    N = _native()
    ctx, key = K.holder(name)
    n, mx = key.n, key.max_int
    lay, ts, x, want = _pack_case(ctx, key, sb, vb, e, dtype)
    k = lay[3]
    ct, st = ctx.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_NONE)
    assert not st.any() and N.words_to_ints(ct) == want
    raws = [(c - 1) // n for c in want]
    assert [t for m in raws for t in unpack(m, n, sb, k)] == ts
    edge = [mx + 1, n // 2, n - mx - 1, mx, n - mx, 1, n - 1]
    status = [N.EL_OVERFLOW if unpack(m, n, sb, k) is None else 0 for m in edge]
    assert status == [N.EL_OVERFLOW] * 5 + [0, 0]
    ect = _words(ctx, [(1 + n * m) % key.nsquare for m in edge])
    was = ctx.rows_max
    try:
        for rows_max in (was, 0):
            ctx.set_rows_max(rows_max)
            for C in (1, PACK_C):
                val, mant, st = ctx.decrypt_packed(ct[:C], lay, C * k)
                assert not st.any(), f"decrypt_packed {name} {lay} rows_max={rows_max} C={C}"
                assert mant.tolist() == ts[:C * k]
                assert val.tolist() == [float(t) * 16.0 ** -e for t in ts[:C * k]]
            val, mant, st = ctx.decrypt_packed(ect, lay, len(edge) * k)
            assert st.reshape(len(edge), k).tolist() == [[s] * k for s in status], (name, rows_max)
            assert mant.reshape(len(edge), k)[5:, 0].tolist() == [1, -1] and not mant.reshape(len(edge), k)[:5].any()
    finally:
        ctx.set_rows_max(was)


# --------------------------------------------------------------------------- 9. pack_ciphertexts
def _fold_case(name, key, sb, k, seed):
    """2 k + 3 inputs under E = 2: (integers, exponents). Output 0 takes unobfuscated ciphertexts 1 + n m of signed
    mantissas that fill their slots, +- alternating, every shift 0 .. sb / 4 - 1 in turn; output 1 random residues with
    empty-segment entries (ciphertext 1, exponent INT32_MIN) among them; output 2 is short."""
    E, dmax = 2, sb // 4 - 1
    mx = (1 << (sb - 1)) - 1
    n_vals = 2 * k + 3
    rnd = _operands(name, key, n_vals, seed)
    cs, es = [], []
    for i in range(n_vals):
        c, j = divmod(i, k)
        d = (j + c) % (dmax + 1)
        if c == 0:
            m = (mx >> (4 * d)) * (1 if j % 2 == 0 else -1)
            cs.append((1 + key.n * (m % key.n)) % key.nsquare)
        elif c == 1 and j % 5 == 2:
            cs.append(1)
            d = None
        else:
            cs.append(rnd[i])
        es.append(EMPTY if d is None else E - d)
    if name in TKEYS:                                        # the top slot opens the Horner chain, slot 0 closes it
        cs[k - 1], cs[0], cs[2 * k - 1], cs[k], cs[-1], cs[2 * k] = _extremes(key)
    return cs, es, E


def _fold_want(cs, es, E, sb, k, key):
    """prod_j c_j^(16^D_j 2^(sb j)) mod n^2 by Horner from the top slot; empty-segment entries are left out."""
    n2, out = key.nsquare, []
    for c0 in range(0, len(cs), k):
        acc = 1
        for c, e in reversed(list(zip(cs[c0:c0 + k], es[c0:c0 + k]))):
            acc = pow(acc, 1 << sb, n2)
            if e != EMPTY:
                acc = acc * pow(c, 16 ** (E - e), n2) % n2
        out.append(acc)
    return out


def _mul_add_chain(ctx, ct, E, sb, k):
    """The route without pai_pack_ciphertexts (test_gpu_fold.py::test_parity_with_the_mul_add_chain) for inputs on one
    exponent: from the top slot down, pai_mul by 2^sb (in steps of at most 2^32) and a 2-way pai_add."""
    C = ct.shape[0] // k
    ex = np.full(C, E, dtype=np.int32)
    rows = ct.reshape(C, k, -1)
    acc = rows[:, k - 1].copy()
    for j in range(k - 2, -1, -1):
        for step in ([32, 32] if sb == 64 else [sb]):
            acc, e1, st = ctx.mul(acc, ex, np.array([1 << step], dtype=np.int64))
            assert not st.any() and np.array_equal(e1, ex)
        acc, e2 = ctx.add([acc, rows[:, j].copy()], [ex, ex])
        assert np.array_equal(e2, ex)
    return acc


@pytest.mark.parametrize("sb", [64, 16])
@pytest.mark.parametrize("name", KEYS)
def test_pack_ciphertexts(K, name, sb):
    """k_pack_fold: sb = 64 at the most slots the key allows, sb = 16 with 40 slots (all of K512's 31); three outputs,
    the last one of three slots."""
    N = _native()
    ctx, key = K.public(name)
    kmax = ctx.pack_max_slots(sb)
    assert kmax == (BITS[name] - 2) // sb
    k = kmax if sb == 64 else min(40, kmax)
    cs, es, E = _fold_case(name, key, sb, k, BITS[name] + sb)
    lay = (sb, sb, E, k)
    out, st = ctx.pack_ciphertexts(_words(ctx, cs), np.array(es, dtype=np.int32), lay)
    assert out.shape == (3, ctx.ct_words) and not st.any()
    got, want = N.words_to_ints(out), _fold_want(cs, es, E, sb, k, key)
    assert got == want, f"pack_ciphertexts {name} sb={sb}: outputs {[c for c in range(3) if got[c] != want[c]]} differ"
    # the same inputs on one exponent, padded with the ciphertext 1 to whole outputs: the library's own mul / add chain
    flat = [1 if e == EMPTY else c for c, e in zip(cs, es)] + [1] * (3 * k - len(cs))
    ct = _words(ctx, flat)
    out, st = ctx.pack_ciphertexts(ct, np.full(3 * k, E, dtype=np.int32), lay)
    assert not st.any() and N.words_to_ints(out) == _fold_want(flat, [E] * (3 * k), E, sb, k, key)
    assert np.array_equal(out, _mul_add_chain(ctx, ct, E, sb, k)), f"pack_ciphertexts {name} sb={sb} vs mul / add"


@pytest.mark.parametrize("name", TKEYS)
def test_pack_ciphertexts_of_the_largest_residue(K, name):
    """Every input n^2 - 1 = -1: only slot 0 with D = 0 has an odd exponent."""
    N = _native()
    ctx, key = K.public(name)
    k = ctx.pack_max_slots(64)
    n2 = key.nsquare
    for es, want in (([2] * k, n2 - 1), ([1] + [2] * (k - 1), 1), ([2] * (k - 1) + [0], n2 - 1)):
        assert _fold_want([n2 - 1] * k, es, 2, 64, k, key) == [want]
        out, st = ctx.pack_ciphertexts(_words(ctx, [n2 - 1] * k), np.array(es, dtype=np.int32), (64, 64, 2, k))
        assert not st.any() and N.words_to_ints(out) == [want], (name, es[0], es[-1])


# --------------------------------------------------------------------------- 10. check_below_dev, take_dev
@pytest.mark.parametrize("name", KEYS)
def test_check_below_dev(K, name):
    """The comparison with n^2 over ct_words words: n^2 - 1 passes at every position; n^2, n^2 + 1 and the all-ones row
    are reported at theirs."""
    N = _native()
    ctx, key = K.public(name)
    W, n2 = ctx.ct_words, key.nsquare
    good = _words(ctx, _operands(name, key, 7, BITS[name] + 10))
    edge = _words(ctx, [n2 - 1, n2, n2 + 1, (1 << (32 * W)) - 1])
    d = N.device_upload(good)
    assert ctx.check_below_dev(d.ptr, 7) == -1
    for row, ok in ((0, True), (1, False), (2, False), (3, False)):
        for pos in range(7):
            words = good.copy()
            words[pos] = edge[row]
            assert ctx.check_below_dev(d.upload(words).ptr, 7) == (-1 if ok else pos), (name, row, pos)


@pytest.mark.parametrize("name", KEYS)
def test_take_dev(K, name):
    """Rows of 65 and 130 words among the widths: a gather with repeats and -1 (ciphertext 1, exponent INT32_MIN)."""
    N = _native()
    ctx, key = K.public(name)
    W = ctx.ct_words
    src = _words(ctx, _operands(name, key, 7, BITS[name] + 11))
    exps = np.arange(7, dtype=np.int32) - 3
    d_ct, d_ex = N.device_upload(src), N.device_upload(exps)
    idx = np.array([6, 0, 0, -1, 3, 6, -1, 5, 0, 6, 1, 2, 4, -1], dtype=np.int64)
    out, oe = N.DeviceMem(idx.size * W * 4, 0), N.DeviceMem(idx.size * 4, 0)
    ctx.take_dev(d_ct.ptr, d_ex.ptr, 7, idx, out.ptr, oe.ptr)
    one = np.zeros(W, dtype=np.uint32)
    one[0] = 1
    want = np.where((idx >= 0)[:, None], src[np.maximum(idx, 0)], one[None, :])
    assert np.array_equal(out.download(np.uint32, idx.size * W).reshape(idx.size, W), want), name
    assert np.array_equal(oe.download(np.int32, idx.size), np.where(idx >= 0, exps[np.maximum(idx, 0)], EMPTY))
    assert np.array_equal(d_ct.download(np.uint32, 7 * W).reshape(7, W), src)
