"""CiphertextBuffer.histogram over an (N, 3) buffer without a GPU: the Python-integer path against the rule itself, the
result shapes and the argument checks."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, C, F, B, NODES = 40, 3, 2, 3, 2


@pytest.fixture(autouse=True)
def no_gpu(monkeypatch):
    from flex.crypto.paillier import _runtime
    monkeypatch.setattr(_runtime, "gpu_available", lambda: False)       # the Python-int path, wherever the suite runs


@pytest.fixture(scope="module")
def buf():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        pk = PaillierPublicKey(int(json.load(f)["keys"]["1024"]["n"], 16))
    rng = np.random.default_rng(3)
    cts = [int.from_bytes(rng.bytes(256), "little") % pk.nsquare for _ in range(N_ * C)]
    W = (2 * pk.n.bit_length() + 31) // 32
    return CiphertextBuffer(pk, _runtime.ints_to_words(cts, W).reshape(-1, W), rng.integers(0, 4, N_ * C), None, (N_, C)), cts


def test_columns_against_the_rule(buf):
    from flex.crypto.paillier import _runtime, parallel_ops
    b, cts = buf
    nsq = b.public_key.nsquare
    rng = np.random.default_rng(4)
    bins = rng.integers(0, B + 1, (N_, F)).astype(np.uint8)         # id B: in no cell
    bins[:, 1] = np.where(bins[:, 1] == 2, 0, bins[:, 1])            # an empty cell in every node
    node = rng.integers(-1, NODES + 1, N_)
    hist, cnt = b.histogram(bins, B, node=node, n_nodes=NODES)
    assert hist.shape == (NODES, F, B, C) and cnt.shape == (NODES, F, B) and not cnt[:, 1, 2].any()
    got = np.array(_runtime.words_to_ints(hist.words), dtype=object).reshape(hist.shape)
    ex = b.exps.reshape(N_, C)
    for v, f, q, c in np.ndindex(*hist.shape):
        mem = np.flatnonzero((node == v) & (bins[:, f] == q)).tolist()
        E = max((int(ex[i, c]) for i in mem), default=0)             # an empty cell reports exponent 0
        acc = 1
        for i in mem:
            acc = acc * pow(cts[i * C + c], 16 ** (E - int(ex[i, c])), nsq) % nsq
        assert cnt[v, f, q] == len(mem) and (got[v, f, q, c], int(hist.exps.reshape(hist.shape)[v, f, q, c])) == (acc, E)
    again, c2 = parallel_ops.histogram(b, bins, B, node=node, n_nodes=NODES)
    assert again.shape == hist.shape and np.array_equal(c2, cnt)
    assert hist.cumsum(axis=2).shape == hist.shape


def test_shapes_and_argument_checks(buf):
    b, _ = buf
    flat, cnt = b.take(np.arange(N_ * C)).histogram(np.zeros((N_ * C, F), dtype=np.uint8), B)
    assert flat.shape == (1, F, B) and cnt.shape == (1, F, B)        # a 1-D buffer keeps today's shape
    wide, cnt = b.histogram(np.zeros((N_ * C, F), dtype=np.uint8), B)
    assert wide.shape == (1, F, B) and cnt[0, 0, 0] == N_ * C        # and so does a 2-D one over N C rows of bins
    with pytest.raises(ValueError):
        b.histogram(np.zeros((N_ + 1, F), dtype=np.uint8), B)        # neither N nor N C rows
    with pytest.raises(ValueError):
        b.histogram(np.zeros((N_, 1), dtype=np.uint16), 65536, node=np.zeros(N_, dtype=np.int64), n_nodes=128)   # 2^23 cells x 3

    class Sparse:                                                    # anything that offers .tocsr() is sparse
        shape = (N_, F)

        def tocsr(self):
            raise AssertionError("refused before it is converted")
    with pytest.raises(TypeError):
        b.histogram(Sparse(), B)
