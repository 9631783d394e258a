"""Encrypted histograms over sparse bins without a GPU: the Python-int fallback of the sparse branch of
parallel_ops.histogram / histogram_packed, CiphertextBuffer.histogram and PackedCiphertextBuffer.histogram against the
reference fixture (tests/golden/paillier_golden_shist.json) and against the dense fallback on the densified matrix, the
duck typing (a minimal CSR stand-in, scipy where installed), the argument checks, the packed buffers' bound rule and
the C ABI's declarations."""
import json
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CSR:
    """What the package needs of a sparse matrix: .tocsr() giving indptr, indices, data and shape."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = np.asarray(indptr), np.asarray(indices), np.asarray(data), shape

    def tocsr(self):
        return self


def densify(csr, default_bin, B):
    """The dense uint16 matrix the sparse one stands for; B marks "in no cell" (a default outside [0, B), a stored id
    >= B)."""
    N, F = csr.shape
    z = np.broadcast_to(np.asarray(default_bin), (F,))
    dense = np.tile(np.where((z >= 0) & (z < B), z, B).astype(np.uint16), (N, 1))
    for i in range(N):
        for t in range(int(csr.indptr[i]), int(csr.indptr[i + 1])):
            dense[i, int(csr.indices[t])] = min(int(csr.data[t]), B)
    return dense


def random_csr(rng, N, F, B, density=0.4):
    indptr, indices, data = [0], [], []
    for _ in range(N):
        fs = np.flatnonzero(rng.random(F) < density)
        indices += fs.tolist()
        data += rng.integers(0, B + 2, fs.size).tolist()           # B and B + 1: missing values
        indptr.append(len(indices))
    return CSR(indptr, indices, data, (N, F))


@pytest.fixture(scope="module")
def gshist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_shist.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def no_gpu():
    from flex.crypto.paillier import _runtime
    mp = pytest.MonkeyPatch()
    mp.setattr(_runtime, "gpu_available", lambda: False)       # the Python-int fallback, wherever the suite runs
    yield
    mp.undo()


@pytest.fixture(scope="module")
def pkg(no_gpu):
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=5)
    return pk, sk, O.Key(pk.n, sk.p, sk.q)


def _buffer(pk, ms, exps=None, seed=3):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    n, nsq = pk.n, pk.nsquare
    W = (2 * n.bit_length() + 31) // 32
    cts = [(1 + n * (int(m) % n)) % nsq * pow(O.golden_r(n, seed, i), n, nsq) % nsq for i, m in enumerate(ms)]
    return CiphertextBuffer(pk, _runtime.ints_to_words(cts, W), np.zeros(len(cts), dtype=np.int32) if exps is None
                            else np.array(exps, dtype=np.int32))


def signed(m, n):
    return m if m <= n // 3 else m - n


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("nb", ["1024", "2048"])
def test_fallback_reproduces_the_fixture(golden, gshist, no_gpu, nb):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.cipher_array import materialize
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    n = int(golden["keys"][nb]["n"], 16)
    pub = PaillierPublicKey(n)
    case, g = gshist["cases"][nb], gshist
    N, F, B, nodes = g["N"], g["F"], g["B"], g["nodes"]
    words = _runtime.ints_to_words([int(h, 16) for h in case["c"]], (2 * n.bit_length() + 31) // 32)
    exps = np.array(case["e"], dtype=np.int32)
    bins = CSR(g["indptr"], g["indices"], g["data"], (N, F))
    node = np.array(g["node"], dtype=np.int32)
    enc = materialize(pub, words, exps, (N,), obfuscated=True)
    arr, cnt = parallel_ops.histogram(enc, bins, B, node, nodes, default_bin=g["default_bin"])
    assert arr.shape == cnt.shape == (nodes, F, B) and cnt.dtype == np.int64
    assert cnt.reshape(-1).tolist() == case["counts"]
    for s, e in enumerate(np.asarray(arr).reshape(-1)):
        if case["cells"][s] is None:
            assert (e.ciphertext(False), e.exponent) == (1, 0)
        else:
            assert [hex(e.ciphertext(False)), e.exponent] == case["cells"][s], (nb, s)
    buf, cnt2 = CiphertextBuffer(pub, words, exps).histogram(bins, B, node, nodes, default_bin=np.array(g["default_bin"]))
    assert buf.shape == (nodes, F, B) and not buf.obfuscated.any() and np.array_equal(cnt2, cnt)
    assert _runtime.words_to_ints(buf.words) == [e.ciphertext(False) for e in np.asarray(arr).reshape(-1)]


# ---------------------------------------------------------------- against the dense fallback
@pytest.mark.parametrize("default_bin", [0, 2, [1, 0, 9, 2, -1]])
def test_uniform_exponents_give_the_dense_bits(pkg, default_bin):
    """One exponent per node: the default cells are bit-identical to the dense histogram of the densified matrix."""
    from flex.crypto.paillier import _runtime
    pk, _, _ = pkg
    rng = np.random.default_rng(11)
    N, F, B, nodes = 60, 5, 3, 2
    csr = random_csr(rng, N, F, B)
    node = rng.integers(-1, nodes + 1, N).astype(np.int32)
    buf = _buffer(pk, rng.integers(-50, 51, N), exps=np.full(N, 4))
    got, c1 = buf.histogram(csr, B, node, nodes, default_bin=default_bin)
    want, c2 = buf.histogram(densify(csr, default_bin, B), B, node, nodes)
    assert np.array_equal(c1, c2) and c1.sum() > 0
    assert _runtime.words_to_ints(got.words) == _runtime.words_to_ints(want.words) and np.array_equal(got.exps, want.exps)


def test_mixed_exponents_decrypt_to_the_dense_values(pkg):
    pk, sk, key = pkg
    from flex.crypto.paillier import _runtime
    rng = np.random.default_rng(12)
    N, F, B = 50, 4, 3
    csr = random_csr(rng, N, F, B, 0.5)
    ms = rng.integers(-1000, 1001, N)
    exps = rng.integers(0, 4, N)
    buf = _buffer(pk, ms, exps=exps)
    got, c1 = buf.histogram(csr, B, default_bin=1)
    want, c2 = buf.histogram(densify(csr, 1, B), B)
    assert np.array_equal(c1, c2)
    gw, ww = _runtime.words_to_ints(got.words), _runtime.words_to_ints(want.words)
    E_T = int(exps.max())
    for s in range(F * B):
        if s % B != 1:
            assert gw[s] == ww[s] and got.exps[s] == want.exps[s]
        elif c1.reshape(-1)[s]:
            # the node's largest exponent, and the dense cell raised to it: the same plaintext
            assert got.exps[s] == E_T >= want.exps[s]
            assert gw[s] == pow(ww[s], 16 ** (E_T - int(want.exps[s])), pk.nsquare)
            assert signed(O.raw_decrypt(gw[s], key), pk.n) == signed(O.raw_decrypt(ww[s], key), pk.n) * 16 ** (E_T - int(want.exps[s]))


def test_scipy_matrices_are_accepted(pkg):
    sp = pytest.importorskip("scipy.sparse")
    from flex.crypto.paillier import _runtime
    pk, _, _ = pkg
    rng = np.random.default_rng(13)
    N, F, B = 40, 6, 2
    onehot = (rng.random((N, F)) < 0.2).astype(np.float64)          # scipy's default dtype, bins 0 / 1
    buf = _buffer(pk, rng.integers(0, 2, N))
    want, c2 = buf.histogram(onehot.astype(np.uint8), B)
    for m in (sp.csr_matrix(onehot), sp.csc_matrix(onehot), sp.coo_matrix(onehot)):
        got, c1 = buf.histogram(m, B)
        assert np.array_equal(c1, c2) and _runtime.words_to_ints(got.words) == _runtime.words_to_ints(want.words)
    # an unsorted CSR operand is canonicalised on a copy
    m = sp.csr_matrix(onehot)
    m.indices[:] = np.concatenate([m.indices[m.indptr[i]:m.indptr[i + 1]][::-1] for i in range(N)])
    m.has_sorted_indices = False
    before = m.indices.copy()
    got, _ = buf.histogram(m, B)
    assert _runtime.words_to_ints(got.words) == _runtime.words_to_ints(want.words) and np.array_equal(m.indices, before)


# ---------------------------------------------------------------- arguments
def test_argument_errors(pkg):
    pk, _, _ = pkg
    buf = _buffer(pk, [1, 2, 3])
    ok = CSR([0, 2, 2, 3], [0, 2, 1], [1, 1, 1], (3, 3))
    out, cnt = buf.histogram(ok, 2)
    assert cnt.reshape(3, 2).tolist() == [[2, 1], [2, 1], [2, 1]]
    with pytest.raises(ValueError, match="strictly increasing"):
        buf.histogram(CSR([0, 2, 2, 3], [2, 0, 1], [1, 1, 1], (3, 3)), 2)           # unsorted
    with pytest.raises(ValueError, match="strictly increasing"):
        buf.histogram(CSR([0, 2, 2, 3], [1, 1, 1], [1, 1, 1], (3, 3)), 2)           # a duplicate
    buf.histogram(CSR([0, 1, 2, 3], [2, 1, 0], [1, 1, 1], (3, 3)), 2)               # decreasing across rows only
    with pytest.raises(IndexError):
        buf.histogram(CSR([0, 2, 2, 3], [0, 3, 1], [1, 1, 1], (3, 3)), 2)
    with pytest.raises(IndexError):
        buf.histogram(CSR([0, 2, 2, 3], [-1, 2, 1], [1, 1, 1], (3, 3)), 2)
    with pytest.raises(ValueError, match="indptr"):
        buf.histogram(CSR([0, 2, 1, 3], [0, 2, 1], [1, 1, 1], (3, 3)), 2)
    with pytest.raises(ValueError, match="indptr"):
        buf.histogram(CSR([1, 2, 2, 3], [0, 2, 1], [1, 1, 1], (3, 3)), 2)
    with pytest.raises(ValueError, match="shape"):
        buf.histogram(CSR([0, 2, 3], [0, 2, 1], [1, 1, 1], (2, 3)), 2)
    with pytest.raises(ValueError, match="default_bin"):
        buf.histogram(ok, 2, default_bin=[0, 1])
    with pytest.raises(ValueError, match="default_bin"):
        buf.histogram(ok, 2, default_bin=0.5)
    with pytest.raises(ValueError, match="integers"):
        buf.histogram(CSR([0, 2, 2, 3], [0, 2, 1], [1.5, 1, 1], (3, 3)), 2)
    with pytest.raises(ValueError, match="negative"):
        buf.histogram(CSR([0, 2, 2, 3], [0, 2, 1], [-1, 1, 1], (3, 3)), 2)
    with pytest.raises(ValueError, match="n_bins"):
        buf.histogram(ok, 0)
    with pytest.raises(ValueError, match="n_bins"):
        buf.histogram(ok, 65537)
    with pytest.raises(ValueError, match="n_nodes"):
        buf.histogram(ok, 2, n_nodes=2)
    with pytest.raises(ValueError, match="cells"):
        buf.histogram(ok, 65536, np.zeros(3, dtype=np.int32), 1 << 10)
    # a dense matrix takes no default_bin other than by keyword, and keeps its own rules
    with pytest.raises(TypeError):
        buf.histogram([[0, 1, 0]] * 3, 2)


def test_bin_dtype_follows_n_bins():
    from flex.crypto.paillier.cipher_buffer import histogram_sparse_args, sparse_csr
    csr = sparse_csr(CSR([0, 2, 3], [0, 2, 1], [1, 300, 70000], (2, 3)))
    for B, dt, ids in ((2, np.uint8, [1, 2, 2]), (255, np.uint8, [1, 255, 255]), (256, np.uint16, [1, 256, 256]),
                       (1000, np.uint16, [1, 300, 1000])):
        _, indices, data, zs, _, shape = histogram_sparse_args(2, csr, B, None, 1, [0, B, -3])
        assert data.dtype == dt and data.tolist() == ids and indices.dtype == np.int32
        assert zs.tolist() == [0, -1, -1] and shape == (1, 3, B)
    with pytest.raises(ValueError, match="missing"):
        histogram_sparse_args(2, csr, 65536, None, 1, 0)


# ---------------------------------------------------------------- packed buffers
def test_packed_bound_rule(pkg, monkeypatch):
    from flex.crypto.paillier import packed_buffer, parallel_ops
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, sk, key = pkg
    rng = np.random.default_rng(14)
    N, F, B, nodes = 40, 4, 2, 2
    csr = random_csr(rng, N, F, B, 0.3)
    node = rng.integers(0, nodes, N).astype(np.int32)
    dense = densify(csr, 0, B)
    y = rng.integers(-1000, 1001, N)
    buf = _buffer(pk, y)
    lay = PackedLayout.for_sum(pk, 1000, 0, N)
    got, c1 = parallel_ops.histogram_packed(buf, csr, B, lay, 1000, node, nodes)
    want, c2 = parallel_ops.histogram_packed(buf, dense, B, lay, 1000, node, nodes)
    # a default cell is a subset sum like any other: counts.max() times the input bound, the dense rule
    assert np.array_equal(c1, c2) and got.bound == want.bound == 1000 * int(c1.max())
    assert np.array_equal(got.words, want.words)
    # a default cell that holds all 40 samples passes a 16-bit slot: refused before the fold, as for dense bins
    folds = []
    monkeypatch.setattr(packed_buffer, "host_pack_ciphertexts", lambda *a, **k: folds.append(1))
    with pytest.raises(OverflowError):
        parallel_ops.histogram_packed(buf, CSR([0] * (N + 1), [], np.zeros(0, dtype=np.uint8), (N, 1)), 1,
                                      PackedLayout(pk, 16, 11, 0), 1000)
    assert not folds


def test_packed_buffer_histogram(pkg, monkeypatch):
    from flex.crypto.paillier import cipher_buffer
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout, host_encrypt_packed
    pk, sk, key = pkg
    rng = np.random.default_rng(15)
    N, F, B = 30, 3, 2
    csr = random_csr(rng, N, F, B, 0.3)
    lay = PackedLayout(pk, 32, 11, 0, 2)
    gh = rng.integers(-1000, 1001, (N, 2)).astype(np.int64)
    words, st = host_encrypt_packed(gh.reshape(-1), lay, pk)
    assert not st.any()
    packed = PackedCiphertextBuffer(pk, words, lay, 2 * N, (N, 2), bound=1000)
    got, c1 = packed.histogram(csr, B, default_bin=0)
    want, c2 = packed.histogram(densify(csr, 0, B), B)
    assert np.array_equal(c1, c2) and got.bound == want.bound == 1000 * int(c1.max())
    assert got.shape == want.shape == (1, F, B, 2) and np.array_equal(got.words, want.words)
    calls = []
    monkeypatch.setattr(cipher_buffer, "histogram_sparse_words", lambda *a, **k: calls.append(1))
    packed.bound = lay.slot_max // 2
    with pytest.raises(OverflowError):
        packed.histogram(csr, B)
    assert not calls


# ---------------------------------------------------------------- the C ABI
def test_c_abi_declares_the_sparse_histogram():
    from flex.crypto.paillier import _native
    with open(os.path.join(ROOT, "include", "flexpai.h")) as f:
        hdr = f.read()
    for name in ("pai_histogram_sparse", "pai_histogram_sparse_dev"):
        assert name in _native.EXPORTED
        assert re.search(r"\bint %s\(pai_ctx\* ctx," % name, hdr)
    assert "WHENEVER THE EXPONENTS OF A NODE ARE" in hdr
