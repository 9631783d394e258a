"""GPU parity of encrypted histograms over a sparse bin matrix (pai_histogram_sparse[_dev]: k_shist_indptr, k_shist_pass
over the stored entries, the member lists through k_hist_acc and the segmented add, the default cells T_v - S_{v,f} through
the batch inversion and a 2-way k_add) against the reference-generated vectors (tests/golden/make_golden_shist.py), the
dense call on the densified matrix, and pai_segment_add + the ciphertext `-` composed from the public calls, bit-exact;
runs, feature blocks and host chunks, the argument errors, and the packed flow down to decrypted values."""
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = -(1 << 31)
N_S, F, B, NODES = 300, 6, 4, 3
DEFAULT = np.array([0, 1, 2, 6, 3, 1], dtype=np.int32)          # feature 3: no default cell


def _native():
    from flex.crypto.paillier import _native as N
    return N


@pytest.fixture(scope="module")
def gshist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_shist.json")) as f:
        return json.load(f)


def _key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def matrix():
    """(indptr, indices, data, node) of the shared 300 x 6 matrix (never written):
    feature 0  one-hot style: default 0, bins 1 .. 3 stored, some explicit default entries, stored ids 4 and 9 (missing)
    feature 1  no stored entry: every default cell is T_v
    feature 2  stored off its default bin 2 for every sample but row 7 (the empty row, in node 1): the default cell of
               node 0 is empty, that of node 1 holds one sample
    feature 3  default_bin 6 >= B: no default cell
    feature 4  bin 0 stored for 260 samples: more than 128 members in one cell of node 0
    feature 5  mostly explicitly stored default entries
    node ids -1 and 3 (out of range) occur, and node 2 is empty."""
    rng = np.random.default_rng(300)
    node = rng.choice(np.array([-1, 0, 0, 0, 0, 0, 0, 1, 1, 3], dtype=np.int32), N_S)
    node[7] = 1
    indptr, indices, data = [0], [], []
    for i in range(N_S):
        row = {}
        if i != 7:
            if rng.random() < 0.5:
                row[0] = int(rng.choice([0, 1, 2, 3, 4, 9]))
            row[2] = int(rng.choice([0, 1, 3]))
            if rng.random() < 0.5:
                row[3] = int(rng.integers(0, B + 1))
            if i < 260:
                row[4] = 0
            elif rng.random() < 0.3:
                row[4] = int(rng.integers(1, B))
            if rng.random() < 0.4:
                row[5] = 1 if rng.random() < 0.8 else int(rng.integers(0, B + 2))
        for f in sorted(row):
            indices.append(f)
            data.append(row[f])
        indptr.append(len(indices))
    m = (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data, dtype=np.uint8), node)
    for a in m:
        a.setflags(write=False)
    assert np.count_nonzero(node[:260] == 0) > 128
    return m


def densify(indptr, indices, data, default=DEFAULT, n_bins=B, n_features=F):
    dense = np.tile(np.where((default >= 0) & (default < n_bins), default, n_bins).astype(np.uint16), (indptr.size - 1, 1))
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    dense[rows, indices] = np.minimum(data, n_bins)
    return dense


def units(key, count, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(key.n.bit_length() // 4), "little") % key.nsquare for _ in range(count)]


@pytest.fixture(scope="module")
def key(golden):
    return _key(golden, 1024)


@pytest.fixture(scope="module")
def ctx(key, xlib):
    """Public key only, on the test build (it reads the run length, the scratch budget and the chunk size from the
    environment)."""
    return _native().Context(key.n, 0, lib=xlib)


@pytest.fixture(scope="module")
def pool(key, ctx):
    """300 random units mod n^2 as ciphertexts with exponents 0 .. 5 (shared, never written)."""
    cs = units(key, N_S, 1024)
    words = _native().ints_to_words(cs, ctx.ct_words)
    exps = np.random.default_rng(2).integers(0, 6, N_S).astype(np.int32)
    words.setflags(write=False)
    exps.setflags(write=False)
    return cs, words, exps


@pytest.fixture(scope="module")
def mixed(ctx, pool, matrix):
    """The sparse histogram of the pool's mixed exponents over the shared matrix, default path (computed once)."""
    _, words, exps = pool
    indptr, indices, data, node = matrix
    got = ctx.histogram_sparse(words, exps, indptr, indices, data, F, DEFAULT, B, node, NODES)
    for a in got:
        a.setflags(write=False)
    return got


# ---------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("nb", [1024, 2048])
def test_fixture_parity(golden, gshist, nb):
    N = _native()
    g, case = gshist, gshist["cases"][str(nb)]
    c = N.Context(_key(golden, nb).n, 0)
    words = N.ints_to_words([int(h, 16) for h in case["c"]], c.ct_words)
    out, oe, cnt = c.histogram_sparse(words, np.array(case["e"], dtype=np.int32), np.array(g["indptr"], dtype=np.int64),
                                      np.array(g["indices"], dtype=np.int32), np.array(g["data"], dtype=np.uint8), g["F"],
                                      np.array(g["default_bin"], dtype=np.int32), g["B"], np.array(g["node"], dtype=np.int32),
                                      g["nodes"])
    assert cnt.tolist() == case["counts"] and cnt.dtype == np.int64
    got = N.words_to_ints(out)
    for s, cell in enumerate(case["cells"]):
        if cell is None:
            assert got[s] == 1 and int(oe[s]) == EMPTY, s
        else:
            assert [hex(got[s]), int(oe[s])] == cell, (nb, s)


# ---------------------------------------------------------------- 2. uniform exponents: the dense call's bits
def _dev_call(c, words, exps, indptr, indices, data, node, with_counts=True):
    import torch
    N = _native()
    dev = torch.device("cuda", 0)
    cells = NODES * F * B
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t = lambda a, view=None: torch.from_numpy(np.array(a).view(view) if view else np.array(a)).to(dev)
        d_ct, d_ex = t(words, np.int32), t(exps)
        d_ptr, d_ind, d_node, d_def = t(indptr), t(indices), t(node), t(DEFAULT)
        d_data = t(data, np.int16) if data.dtype == np.uint16 else t(data)
        d_out = torch.empty((cells, c.ct_words), dtype=torch.int32, device=dev)
        d_oe = torch.empty(cells, dtype=torch.int32, device=dev)
        d_cnt = torch.empty(cells, dtype=torch.int64, device=dev)
        rc = c.lib.pai_histogram_sparse_dev(c.handle, d_ct.data_ptr(), d_ex.data_ptr(), exps.size, d_ptr.data_ptr(),
                                            d_ind.data_ptr(), N.PAI_BIN_U16 if data.dtype == np.uint16 else N.PAI_BIN_U8,
                                            d_data.data_ptr(), F, d_def.data_ptr(), d_node.data_ptr(), NODES, B,
                                            d_out.data_ptr(), d_oe.data_ptr(), d_cnt.data_ptr() if with_counts else None,
                                            stream.cuda_stream)
        stream.synchronize()
        return rc, d_out.cpu().numpy().view(np.uint32), d_oe.cpu().numpy(), d_cnt.cpu().numpy()


@pytest.mark.parametrize("nb", [1024, 2048, 4096])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_uniform_exponents_equal_the_dense_call(golden, matrix, nb, dtype):
    """TPI 2 / 4 / 8. One exponent for all samples: every cell, the default ones included, and every count is
    bit-identical to pai_histogram on the densified matrix, from the host and from the device variant."""
    N = _native()
    key = _key(golden, nb)
    c = N.Context(key.n, 0)
    indptr, indices, data, node = matrix
    data = data.astype(dtype)
    words = N.ints_to_words(units(key, N_S, nb), c.ct_words)
    exps = np.full(N_S, 3, dtype=np.int32)
    want, we, wc = c.histogram(words, exps, densify(indptr, indices, data).astype(dtype), B, node, NODES)
    at = lambda v, f, b: (v * F + f) * B + b
    assert wc[at(0, 4, 0)] > 128 and wc[at(0, 2, 2)] == 0 and wc[at(1, 2, 2)] == 1 and not wc[at(2, 0, 0):].any()
    got, ge, gc = c.histogram_sparse(words, exps, indptr, indices, data, F, DEFAULT, B, node, NODES)
    assert np.array_equal(gc, wc) and np.array_equal(ge, we) and np.array_equal(got, want)
    rc, dout, doe, dcnt = _dev_call(c, words, exps, indptr, indices, data, node)
    assert rc == 0 and np.array_equal(dcnt, wc) and np.array_equal(doe, we) and np.array_equal(dout, want)
    # feature 1 has no stored entry: its default cells are T_v, what the dense call sums over the whole node
    tw, te = c.segment_add(words, exps, np.flatnonzero(node == 1).astype(np.int64), np.array([0, wc[at(1, 1, 1)]], dtype=np.int64))
    assert np.array_equal(got[at(1, 1, 1)], tw[0]) and ge[at(1, 1, 1)] == te[0]


def test_dev_variant_without_counts(ctx, pool, matrix, mixed):
    _, words, exps = pool
    for _ in range(2):                                          # a second call on the same context
        rc, dout, doe, _ = _dev_call(ctx, words, exps, *matrix, with_counts=False)
        assert rc == 0 and np.array_equal(dout, mixed[0]) and np.array_equal(doe, mixed[1])


# ---------------------------------------------------------------- 3. mixed exponents
def test_mixed_exponents(key, ctx, pool, matrix, mixed):
    """Cells off the default bin: the dense call's bits. Default cells: pai_segment_add for T_v and S_{v,f}, pai_mul by
    -1 and pai_add (the ciphertext `-`), bit for bit, at the node's largest exponent; they decrypt to the dense cell's
    value."""
    N = _native()
    cs, words, exps = pool
    indptr, indices, data, node = matrix
    out, oe, cnt = mixed
    dense = densify(indptr, indices, data)
    want, we, wc = ctx.histogram(words, exps, dense, B, node, NODES)
    assert np.array_equal(cnt, wc)
    at = lambda v, f, b: (v * F + f) * B + b
    rows = np.repeat(np.arange(N_S), np.diff(indptr))
    checked = inverted = 0
    for v in range(NODES):
        members = np.flatnonzero(node == v)
        for f in range(F):
            z = int(DEFAULT[f])
            for b in range(B):
                s = at(v, f, b)
                if b != z:
                    assert np.array_equal(out[s], want[s]) and oe[s] == we[s], (v, f, b)
                    continue
                if cnt[s] == 0:
                    assert N.words_to_ints(out[s:s + 1]) == [1] and oe[s] == EMPTY
                    continue
                t = np.flatnonzero((indices == f) & (data != z))
                rest = t[node[rows[t]] == v]
                off = np.array([0, members.size, members.size + rest.size], dtype=np.int64)
                ts, te = ctx.segment_add(words, exps, np.concatenate([members, rows[rest]]).astype(np.int64), off)
                if rest.size:
                    neg, ne, _ = ctx.mul(ts[1:2], te[1:2], np.array([-1], dtype=np.int64))
                    comp, ce = ctx.add([ts[0:1], neg], [te[0:1], ne])
                    inverted += 1
                else:
                    comp, ce = ts[0:1], te[0:1]
                assert np.array_equal(out[s], comp[0]) and oe[s] == ce[0] == exps[members].max(), (v, f)
                # the dense cell raised to the node's exponent: the same plaintext
                up = 16 ** (int(oe[s]) - int(we[s]))
                assert N.words_to_ints(out[s:s + 1])[0] == pow(N.words_to_ints(want[s:s + 1])[0], up, key.nsquare)
                checked += 1
    assert checked >= 8 and inverted >= 6
    s = at(0, 0, 0)
    assert O.raw_decrypt(N.words_to_ints(out[s:s + 1])[0], key) == \
        O.raw_decrypt(N.words_to_ints(want[s:s + 1])[0], key) * 16 ** (int(oe[s]) - int(we[s])) % key.n


# ---------------------------------------------------------------- 4. runs, feature blocks, host chunks
HIST_ENV = ("FLEXPAI_HIST_ACC", "FLEXPAI_HIST_RUN", "FLEXPAI_HIST_SCRATCH_BYTES", "FLEXPAI_HIST_CHUNK")


@pytest.mark.parametrize("env", [{"FLEXPAI_HIST_RUN": "7"}, {"FLEXPAI_HIST_RUN": "64"}, {"FLEXPAI_HIST_ACC": "0"},
                                 {"FLEXPAI_HIST_SCRATCH_BYTES": "1500"},
                                 {"FLEXPAI_HIST_SCRATCH_BYTES": "1", "FLEXPAI_HIST_CHUNK": "70", "FLEXPAI_HIST_RUN": "7"}])
def test_paths_give_the_same_bits(ctx, pool, matrix, mixed, monkeypatch, env):
    """Runs of 7 and 64, k_add over gather rows, feature blocks of a few features and of one, five chunks of samples (the
    last ragged): no bit changes, the default cells included, because the subtraction follows the combined slot sums."""
    _, words, exps = pool
    for k in HIST_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                               # read by the test build only, at every call
    got = ctx.histogram_sparse(words, exps, *matrix[:3], F, DEFAULT, B, matrix[3], NODES)
    for a, b in zip(got, mixed):
        assert np.array_equal(a, b), env


# ---------------------------------------------------------------- 5. errors
def test_argument_errors(ctx, pool):
    N = _native()
    _, words, exps = pool
    w, e = np.ascontiguousarray(words[:4]), np.ascontiguousarray(exps[:4])
    out = np.empty((3 * 2, ctx.ct_words), dtype=np.uint32)
    oe = np.empty(6, dtype=np.int32)
    node = np.zeros(4, dtype=np.int32)
    zs = np.zeros(3, dtype=np.int32)
    good = (np.array([0, 2, 2, 3, 4], dtype=np.int64), np.array([0, 2, 1, 0], dtype=np.int32))
    vals = np.ones(4, dtype=np.uint8)

    def call(ptr=good[0], ind=good[1], n_feat=3, nd=None, nodes=1, n_bins=2, dt=N.PAI_BIN_U8, n=4, o=out.ctypes.data,
             z=zs.ctypes.data):
        return ctx.lib.pai_histogram_sparse(ctx.handle, w.ctypes.data, e.ctypes.data, n, None if ptr is None else ptr.ctypes.data,
                                            None if ind is None else ind.ctypes.data, dt, vals.ctypes.data, n_feat, z, nd, nodes,
                                            n_bins, o, oe.ctypes.data, None)
    i64, i32 = (lambda *a: np.array(a, dtype=np.int64)), (lambda *a: np.array(a, dtype=np.int32))
    assert call() == 0
    assert call(ptr=None) == -1 and call(ind=None) == -1 and call(o=None) == -1 and call(z=None) == -1
    assert call(n_feat=0) == -1 and call(n_bins=0) == -1 and call(n_bins=257) == -1 and call(dt=2) == -1
    assert call(dt=N.PAI_BIN_U16, n_bins=65537, n_feat=1, ind=i32(0, 0, 0, 0), ptr=i64(0, 1, 2, 3, 4)) == -1
    assert call(nodes=0) == -1 and call(nodes=2) == -1
    assert call(nd=node.ctypes.data, nodes=1 << 23) == -1                   # 2^23 x 3 x 2 cells
    assert call(ptr=i64(0, 2, 1, 3, 4)) == -1 and "indptr" in ctx.lib.pai_last_error().decode()
    assert call(ptr=i64(1, 2, 2, 3, 4)) == -1
    assert call(ptr=i64(0, 2, 2, 3, 1 << 31)) == -1 and "nnz" in ctx.lib.pai_last_error().decode()
    assert call(ind=i32(0, 3, 1, 0)) == -1 and "index" in ctx.lib.pai_last_error().decode()
    assert call(ind=i32(0, -1, 1, 0)) == -1
    # unsorted and duplicate indices inside a row: an error from the counting pass, and no fault
    assert call(ind=i32(2, 0, 1, 0)) == -1 and "strictly increasing" in ctx.lib.pai_last_error().decode()
    assert call(ind=i32(1, 1, 1, 0)) == -1 and "strictly increasing" in ctx.lib.pai_last_error().decode()
    assert call(ind=i32(0, 2, 0, 0)) == 0                                   # decreasing across rows only
    assert call() == 0


def test_dev_variant_reports_a_bad_matrix(ctx, pool, matrix):
    _, words, exps = pool
    indptr, indices, data, node = matrix
    bad = indices.copy()
    bad[[0, 1]] = bad[[1, 0]]                                   # row 0 holds two entries or more
    assert indptr[1] >= 2
    assert _dev_call(ctx, words, exps, indptr, bad, data, node)[0] == -1
    bad = indptr.copy()
    bad[5] = bad[6] + 1
    assert _dev_call(ctx, words, exps, bad, indices, data, node)[0] == -1
    bad = indices.copy()
    bad[-1] = F
    assert _dev_call(ctx, words, exps, indptr, bad, data, node)[0] == -1


# ---------------------------------------------------------------- 6. the package, downstream
class CSR:
    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape

    def tocsr(self):
        return self


@pytest.fixture(scope="module")
def party():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=37)
    yield pk, PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    # this key's cached context must not outlive the module (see test_gpu_fold.test_package_segment_sum_packed)
    with _runtime._lock:
        for k in [k for k in _runtime._ctxs if k[0] == pk.n]:
            _runtime._ctxs.pop(k).close()
        _runtime._private.pop(pk.n, None)


def plain_hist(vals, bins, node):
    out = np.zeros((NODES, F, B) + vals.shape[1:], dtype=np.int64)
    ok = (node >= 0) & (node < NODES)
    for f in range(F):
        sel = ok & (bins[:, f] < B)
        np.add.at(out, (node[sel], f, bins[sel, f].astype(np.int64)), vals[sel])
    return out


def test_packed_flow_downstream(party, matrix):
    """(g, h) packed per sample -> histogram(sparse) -> cumsum -> to_wire(be_secure=True) -> decrypt: plain numpy on the
    densified bins."""
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, enc, dec = party
    indptr, indices, data, node = matrix
    rng = np.random.default_rng(9)
    gh = rng.integers(-1000, 1001, (N_S, 2)).astype(np.int64)
    lay = PackedLayout(pk, 32, 11, 0, 2)
    src = enc.encrypt_packed(gh, lay)
    src.bound = 1000
    bins = CSR(indptr, indices, data, (N_S, F))
    hist, cnt = src.histogram(bins, B, node, NODES, default_bin=DEFAULT)
    dense = densify(indptr, indices, data)
    want = plain_hist(gh, dense, node)
    assert hist.shape == (NODES, F, B, 2) and hist.bound == 1000 * int(cnt.max())
    assert np.array_equal(cnt, plain_hist(np.ones(N_S, dtype=np.int64), dense, node))
    # a packed buffer's exponents are uniform: the dense call's bits
    ref, c2 = src.histogram(dense, B, node, NODES)
    assert np.array_equal(hist.words, ref.words) and np.array_equal(cnt, c2)
    left = hist.cumsum(2)
    wire = left.to_wire(be_secure=True)
    back = PackedCiphertextBuffer.from_wire(wire, pk)
    assert np.asarray(dec.decrypt(back)).reshape(NODES, F, B, 2).tolist() == np.cumsum(want, axis=2).tolist()
    # the plain buffer and a scalar default_bin
    y = rng.integers(0, 2, N_S).astype(np.int64)
    arr, c3 = enc.encrypt_to_buffer(y).histogram(bins, B, node, NODES, default_bin=1)
    d1 = densify(indptr, indices, data, np.full(F, 1, dtype=np.int32))
    assert np.asarray(dec.decrypt(arr)).reshape(NODES, F, B).tolist() == plain_hist(y, d1, node).tolist()
    assert np.array_equal(c3, plain_hist(np.ones(N_S, dtype=np.int64), d1, node))
