"""Segmented weighted sums without a GPU: the Python-integer path of CiphertextBuffer.segment_dot, the sparse operand
of .dot / @ and parallel_ops.segment_dot, against the reference-generated vectors
(tests/golden/make_golden_segdot.py) and the per-object operators. gpu_available() is patched to False, so the same
tests take the same path on a machine that has a GPU."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gsd():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_segdot.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _no_gpu(monkeypatch):
    from flex.crypto.paillier import _runtime
    monkeypatch.setattr(_runtime, "gpu_available", lambda: False)


def _weights(g, name):
    return (np.array([float.fromhex(v) for v in g["weights"][name]]) if name == "f64"
            else np.array(g["weights"][name], dtype=np.int64))


def _buffer(golden, g, nb):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    pk = PaillierPublicKey(int(golden["keys"][str(nb)]["n"], 16))
    W = (2 * pk.n.bit_length() + 31) // 32
    words = _runtime.ints_to_words([int(h, 16) for h in g["c"]], W)
    return CiphertextBuffer(pk, words, np.array(g["e"], dtype=np.int32))


def _pairs(buf):
    from flex.crypto.paillier import _runtime
    return list(zip(_runtime.words_to_ints(buf.words), (int(e) for e in buf.exps)))


@pytest.mark.parametrize("name", ["f64", "i64"])
@pytest.mark.parametrize("nb", [1024, 2048])
def test_integer_path_equals_the_reference(golden, gsd, nb, name):
    g = gsd["cases"][str(nb)]
    buf = _buffer(golden, g, nb)
    out = buf.segment_dot(g["index"], g["seg_off"], _weights(g, name))
    assert out.shape == (len(g["seg_off"]) - 1,)
    want = [(1, 0) if w is None else (int(w[0], 16), w[1]) for w in g["out"][name]]
    assert g["out"][name][0] is None and _pairs(out) == want
    assert not out.obfuscated.any()


def test_argument_errors(golden, gsd):
    g = gsd["cases"]["1024"]
    buf = _buffer(golden, g, 1024)
    w = np.ones(3)
    with pytest.raises(IndexError):
        buf.segment_dot([0, 1, buf.size], [0, 3], w)
    with pytest.raises(IndexError):
        buf.segment_dot([0, -1, 2], [0, 3], w)
    with pytest.raises(ValueError):
        buf.segment_dot([0, 1, 2], [0, 2, 1, 3], w)                  # decreasing
    with pytest.raises(ValueError):
        buf.segment_dot([0, 1, 2], [1, 3], w)                        # does not start at 0
    with pytest.raises(ValueError):
        buf.segment_dot([0, 1, 2], [0, 2], w)                        # does not end at nnz
    with pytest.raises(ValueError):
        buf.segment_dot([0, 1, 2], [0, 3], np.ones(2))
    with pytest.raises(TypeError):
        buf.segment_dot([0, 1, 2], [0, 3], np.array(["a", "b", "c"]))
    with pytest.raises(TypeError):
        buf.segment_dot([0.5, 1, 2], [0, 3], w)
    with pytest.raises(ValueError, match="index 1 "):
        buf.segment_dot([0, 1, 2], [0, 3], np.array([1.0, np.nan, np.nan]))
    assert buf.segment_dot([], [0], np.zeros(0)).shape == (0,)


class _OnlyCsc:
    """What the package may rely on: .tocsc() and, on its result, indptr / indices / data / shape."""

    def __init__(self, indptr, indices, data, shape):
        self._v = (indptr, indices, data, shape)

    def tocsc(self):
        class V:
            pass
        v = V()
        v.indptr, v.indices, v.data, v.shape = self._v
        return v


def _sparse_case():
    """(K, d) = (6, 4): an explicit zero in column 0, column 2 empty, a negative and a repeated row."""
    indptr = [0, 3, 4, 4, 7]
    indices = [0, 2, 5, 1, 0, 3, 4]
    data = [1.5, 0.0, -2.0, 3.0, 0.25, -1.0, 7.0]
    return indptr, indices, data, (6, 4)


@pytest.mark.parametrize("m", [None, 2])
def test_sparse_dot_shapes_zeros_and_empty_column(golden, gsd, m):
    import scipy.sparse as sp
    from flex.crypto.paillier.cipher_array import materialize
    g = gsd["cases"]["1024"]
    full = _buffer(golden, g, 1024)
    K, d = 6, 4
    rows = m or 1
    buf = type(full)(full.public_key, full.words[:rows * K], full.exps[:rows * K], shape=(rows, K) if m else (K,))
    indptr, indices, data, shape = _sparse_case()
    csc = sp.csc_matrix((np.array(data), np.array(indices), np.array(indptr)), shape=shape)
    assert csc.nnz == 7                                              # the stored zero is an entry
    duck = _OnlyCsc(np.array(indptr), np.array(indices), np.array(data), shape)
    want_shape = (m, d) if m else (d,)
    # the reference's own loop over the stored entries
    objs = np.asarray(buf.to_array()).reshape(rows, K)
    want = []
    for i in range(rows):
        for j in range(d):
            acc = None
            for t in range(indptr[j], indptr[j + 1]):
                term = objs[i, indices[t]] * data[t]
                acc = term if acc is None else acc + term
            want.append((1, 0) if acc is None else (acc.ciphertext(False), acc.exponent))
    for operand in (csc, csc.tocsr(), duck):
        out = buf.dot(operand)
        assert out.shape == want_shape and _pairs(out) == want
        out = buf @ operand
        assert _pairs(out) == want
    # column 0 keeps its explicit zero as a term (ciphertext 1 at exp + e(0.0)), column 2 is empty
    z = objs[0, 2] * 0.0
    assert z.ciphertext(False) == 1 and want[0][1] >= z.exponent
    assert want[2] == (1, 0)                                         # the empty column
    # PaillierArray: the same bits, as objects
    arr = materialize(buf.public_key, buf.words, buf.exps, buf.shape, obfuscated=False)
    for res in (arr.dot(csc), arr @ duck):
        assert res.shape == want_shape
        assert [(e.ciphertext(False), e.exponent) for e in np.asarray(res).reshape(-1)] == want
    with pytest.raises(ValueError):
        buf.dot(sp.csc_matrix((K + 1, d)))


def test_dense_operands_keep_their_route(golden, gsd):
    """A dense ndarray never reaches the sparse branch (and without a GPU the buffer's dense dot still refuses)."""
    from flex.crypto.paillier.cipher_buffer import sparse_csc
    assert sparse_csc(np.zeros((3, 2))) is None and sparse_csc([[1.0]]) is None
    buf = _buffer(golden, gsd["cases"]["1024"], 1024)
    with pytest.raises(RuntimeError):
        buf.dot(np.ones(buf.size))


def test_parallel_ops_segment_dot(golden, gsd):
    from flex.crypto.paillier import parallel_ops
    g = gsd["cases"]["1024"]
    buf = _buffer(golden, g, 1024)
    objs = np.asarray(buf.to_array())
    lists = [[0, 5, 5], [], [23, -1], [7]]
    weights = [[1.5, -2.0, 0.0], [], [3, 4], [-1]]
    got = parallel_ops.segment_dot(objs, lists, [np.array(w, dtype=np.float64) for w in weights])
    want = [sum(objs[i] * float(w) for i, w in zip(idx, ws)) for idx, ws in zip(lists, weights)]
    assert got[1] == 0 and want[1] == 0
    for a, b in zip(got, want):
        if not isinstance(b, int):
            assert (a.ciphertext(False), a.exponent) == (b.ciphertext(False), b.exponent)
    assert parallel_ops.segment_dot(np.array([1.0, 2.0, 3.0]), [[0, 2], []], [[2.0, 1.0], []]) == [5.0, 0]
    with pytest.raises(ValueError):
        parallel_ops.segment_dot(objs, [[0, 1]], [[1.0]])
