"""Encrypted histograms without a GPU: the Python-int fallbacks of parallel_ops.histogram, histogram_packed and
PackedCiphertextBuffer.histogram against the reference fixture (tests/golden/paillier_golden_hist.json) and against
np.add.at over the plain values, the argument errors, the overflow refusal, and the C ABI's declarations."""
import json
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ghist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_hist.json")) as f:
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


def signed(m, n):
    return m if m <= n // 3 else m - n


def plain_hist(vals, bins, B, node, nodes):
    """np.add.at over the cell rule: sums [nodes, F, B] and counts."""
    N, F = bins.shape
    sums = np.zeros((nodes, F, B), dtype=np.int64)
    cnt = np.zeros((nodes, F, B), dtype=np.int64)
    v = np.zeros(N, dtype=np.int64) if node is None else np.asarray(node, dtype=np.int64)
    for f in range(F):
        ok = (bins[:, f] < B) & (v >= 0) & (v < nodes)
        np.add.at(sums, (v[ok], f, bins[ok, f].astype(np.int64)), np.asarray(vals, dtype=np.int64)[ok])
        np.add.at(cnt, (v[ok], f, bins[ok, f].astype(np.int64)), 1)
    return sums, cnt


def _buffer(pk, ms, exps=None, seed=3):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    n, nsq = pk.n, pk.nsquare
    W = (2 * n.bit_length() + 31) // 32
    cts = [(1 + n * (int(m) % n)) % nsq * pow(O.golden_r(n, seed, i), n, nsq) % nsq for i, m in enumerate(ms)]
    return CiphertextBuffer(pk, _runtime.ints_to_words(cts, W), np.zeros(len(cts), dtype=np.int32) if exps is None
                            else np.array(exps, dtype=np.int32))


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", ["labels", "floats"])
def test_fallback_reproduces_the_fixture(golden, ghist, no_gpu, name):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.cipher_array import materialize
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    n = int(golden["keys"]["1024"]["n"], 16)
    pub = PaillierPublicKey(n)
    case = ghist["cases"][name]
    F, B, nodes = ghist["F"], ghist["B"], ghist["nodes"]
    words = _runtime.ints_to_words([int(h, 16) for h in case["c"]], (2 * n.bit_length() + 31) // 32)
    exps = np.array(case["e"], dtype=np.int32)
    bins = np.array(ghist["bins"], dtype=np.uint8)
    node = np.array(ghist["node"], dtype=np.int32)
    enc = materialize(pub, words, exps, (len(case["c"]),), obfuscated=True)
    arr, cnt = parallel_ops.histogram(enc, bins, B, node, nodes)
    assert arr.shape == cnt.shape == (nodes, F, B) and cnt.dtype == np.int64
    assert cnt.reshape(-1).tolist() == case["counts"]
    for s, e in enumerate(np.asarray(arr).reshape(-1)):
        if case["cells"][s] is None:
            assert (e.ciphertext(False), e.exponent) == (1, 0)
        else:
            assert [hex(e.ciphertext(False)), e.exponent] == case["cells"][s], (name, s)
    # the buffer method and a row-strided uint16 matrix give the same bits
    wide = np.zeros((len(case["c"]), F + 2), dtype=np.uint16)
    wide[:, :F] = bins
    buf, cnt2 = CiphertextBuffer(pub, words, exps).histogram(wide[:, :F], B, node, nodes)
    assert buf.shape == (nodes, F, B) and not buf.obfuscated.any() and np.array_equal(cnt2, cnt)
    assert _runtime.words_to_ints(buf.words) == [e.ciphertext(False) for e in np.asarray(arr).reshape(-1)]


def test_packed_fallback_on_the_fixture_labels(golden, ghist, no_gpu):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_decrypt_packed, host_pack_ciphertexts

    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    pub = PaillierPublicKey(key.n)
    case = ghist["cases"]["labels"]
    F, B, nodes = ghist["F"], ghist["B"], ghist["nodes"]
    words = _runtime.ints_to_words([int(h, 16) for h in case["c"]], (2 * key.n.bit_length() + 31) // 32)
    bins = np.array(ghist["bins"], dtype=np.uint8)
    node = np.array(ghist["node"], dtype=np.int32)
    lay = PackedLayout.for_sum(pub, 1, 0, 48)
    buf, cnt = parallel_ops.histogram_packed(CiphertextBuffer(pub, words, np.zeros(48, dtype=np.int32)), bins, B, lay, 1,
                                             node, nodes)
    assert buf.shape == (nodes, F, B) and buf.bound == max(case["counts"]) and cnt.reshape(-1).tolist() == case["counts"]
    # the fold of the reference's cell sums (the empty cells fold as 1)
    cells = [1 if c is None else int(c[0], 16) for c in case["cells"]]
    exps = [-(1 << 31) if c is None else c[1] for c in case["cells"]]
    want, st = host_pack_ciphertexts(cells, exps, lay, pub)
    assert _runtime.words_to_ints(buf.words) == want and not st.any()
    sums, _ = plain_hist(case["x"], bins, B, node, nodes)
    got = [v for c in want for v in _unpack(O.raw_decrypt(c, key), key.n, lay.slot_bits, lay.slots)][:buf.count]
    assert got == sums.reshape(-1).tolist()


def _unpack(m, n, sb, k):
    M = signed(m, n)
    Bs, out = 1 << sb, []
    for _ in range(k):
        t = ((M + Bs // 2) % Bs) - Bs // 2
        out.append(t)
        M = (M - t) // Bs
    assert M == 0
    return out


# ---------------------------------------------------------------- values against np.add.at
@pytest.mark.parametrize("dtype,B,nodes", [(np.uint8, 5, 1), (np.uint8, 256, 3), (np.uint16, 300, 2)])
def test_fallback_values(pkg, dtype, B, nodes):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_decrypt_packed
    pk, sk, key = pkg
    rng = np.random.default_rng(B)
    N, F = 90, 2
    vals = rng.integers(-50, 51, N)
    bins = rng.integers(0, min(B, 6) + 1, (N, F)).astype(dtype)
    bins[0, 0] = B - 1
    bins[1, 1] = min(B, np.iinfo(dtype).max)                   # missing where the type can say so
    node = None if nodes == 1 else rng.integers(-1, nodes + 1, N)
    sums, cnt = plain_hist(vals, bins, B, node, nodes)
    buf = _buffer(pk, vals)
    out, c1 = buf.histogram(bins, B, node, nodes)
    assert np.array_equal(c1, cnt) and out.shape == (nodes, F, B)
    got = [signed(O.raw_decrypt(c, key), key.n) for c in _runtime.words_to_ints(out.words)]
    assert got == sums.reshape(-1).tolist() and not out.exps.any()
    # packed reply
    lay = PackedLayout.for_sum(pk, 50, 0, N)
    pbuf, c2 = parallel_ops.histogram_packed(buf, bins, B, lay, 50, node, nodes)
    assert np.array_equal(c2, cnt) and pbuf.bound == int(cnt.max()) * 50
    assert host_decrypt_packed(pbuf, sk) == sums.reshape(-1).tolist()


def test_packed_samples_fallback(pkg):
    """(g, h) of a sample in two slots of one ciphertext: both plain histograms come back."""
    from flex.crypto.paillier.packed_buffer import (PackedCiphertextBuffer, PackedLayout, host_decrypt_packed,
                                                    host_encrypt_packed)
    pk, sk, key = pkg
    rng = np.random.default_rng(8)
    N, F, B, nodes = 60, 3, 4, 2
    gh = rng.integers(-1000, 1001, (N, 2)).astype(np.int64)
    bins = rng.integers(0, B + 1, (N, F)).astype(np.uint8)
    node = rng.integers(-1, nodes + 1, N).astype(np.int32)
    lay = PackedLayout(pk, 32, 11, 0, 2)
    words, st = host_encrypt_packed(gh.reshape(-1), lay, pk)
    assert not st.any()
    src = PackedCiphertextBuffer(pk, words, lay, 2 * N, (N, 2), bound=1000)
    out, cnt = src.histogram(bins, B, node, nodes)
    sg, c0 = plain_hist(gh[:, 0], bins, B, node, nodes)
    sh, _ = plain_hist(gh[:, 1], bins, B, node, nodes)
    assert np.array_equal(cnt, c0) and out.shape == (nodes, F, B, 2) and out.count == nodes * F * B * 2
    assert out.layout == lay and out.bound == 1000 * int(c0.max()) and not out.obfuscated
    got = np.array(host_decrypt_packed(out, sk), dtype=np.int64).reshape(nodes, F, B, 2)
    assert np.array_equal(got[..., 0], sg) and np.array_equal(got[..., 1], sh)
    # a buffer that is not one ciphertext per sample is refused
    with pytest.raises(ValueError, match="one ciphertext"):
        PackedCiphertextBuffer(pk, words[:N // 2 + 1], lay, N + 1, bound=1000).histogram(bins[:N // 2 + 1], B)


# ---------------------------------------------------------------- errors
def test_argument_errors(pkg):
    from flex.crypto.paillier import parallel_ops
    pk, sk, key = pkg
    buf = _buffer(pk, [1, 2, 3, 4])
    ok = np.zeros((4, 2), dtype=np.uint8)
    with pytest.raises(TypeError, match="bins"):
        buf.histogram(ok.astype(np.int32), 2)
    with pytest.raises(TypeError, match="bins"):
        buf.histogram(ok.tolist(), 2)
    with pytest.raises(ValueError, match="bins"):
        buf.histogram(ok[:3], 2)
    with pytest.raises(ValueError, match="bins"):
        buf.histogram(ok.reshape(-1), 2)
    with pytest.raises(ValueError, match="bins"):
        buf.histogram(np.zeros((4, 6), dtype=np.uint8)[:, ::2], 2)          # strided inside a row
    with pytest.raises(ValueError, match="bins"):
        buf.histogram(np.asfortranarray(ok), 2)
    with pytest.raises(ValueError, match="n_bins"):
        buf.histogram(ok, 0)
    with pytest.raises(ValueError, match="n_bins"):
        buf.histogram(ok, 257)
    with pytest.raises(ValueError, match="n_bins"):
        buf.histogram(ok.astype(np.uint16), 65537)
    with pytest.raises(TypeError, match="n_bins"):
        buf.histogram(ok, 2.0)
    with pytest.raises(ValueError, match="n_nodes"):
        buf.histogram(ok, 2, None, 2)
    with pytest.raises(ValueError, match="n_nodes"):
        buf.histogram(ok, 2, np.zeros(4, dtype=np.int32), 0)
    with pytest.raises(ValueError, match="node"):
        buf.histogram(ok, 2, np.zeros(3, dtype=np.int32), 1)
    with pytest.raises(TypeError, match="node"):
        buf.histogram(ok, 2, np.zeros(4), 1)
    with pytest.raises(ValueError, match="cells"):
        buf.histogram(ok.astype(np.uint16), 65536, np.zeros(4, dtype=np.int32), 129)
    with pytest.raises(TypeError, match="histogram"):
        parallel_ops.histogram(np.array([1.0, 2.0]), ok[:2], 2)
    # a strided matrix with contiguous rows is fine, and so is a uint64 node id beyond the range
    out, cnt = buf.histogram(np.zeros((4, 6), dtype=np.uint8)[:, :2], 2, np.array([0, 1, 2 ** 40, 0], dtype=np.uint64), 2)
    assert cnt.tolist() == [[[2, 0], [2, 0]], [[1, 0], [1, 0]]]


def test_overflow_is_refused_before_the_fold(pkg, monkeypatch):
    from flex.crypto.paillier import packed_buffer, parallel_ops
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout, host_encrypt_packed
    pk, sk, key = pkg
    N = 40
    buf = _buffer(pk, [1000] * N)
    bins = np.zeros((N, 1), dtype=np.uint8)                    # one cell holds every sample
    lay = PackedLayout(pk, 16, 11, 0)                          # slot_max 32767 < 40 * 1000
    folds = []
    monkeypatch.setattr(packed_buffer, "host_pack_ciphertexts", lambda *a, **k: folds.append(1))
    with pytest.raises(OverflowError):
        parallel_ops.histogram_packed(buf, bins, 1, lay, 1000)
    assert not folds
    # 20 samples per cell fit
    bins[N // 2:, 0] = 1
    monkeypatch.undo()
    out, cnt = parallel_ops.histogram_packed(buf, bins, 2, lay, 1000)
    assert out.bound == 20000 and cnt.reshape(-1).tolist() == [20, 20]
    # packed samples: refused before the histogram itself runs
    lay2 = PackedLayout(pk, 16, 11, 0, 2)
    words, _ = host_encrypt_packed(np.full(2 * N, 1000, dtype=np.int64), lay2, pk)
    src = PackedCiphertextBuffer(pk, words, lay2, 2 * N, bound=1000)
    from flex.crypto.paillier import cipher_buffer
    calls = []
    monkeypatch.setattr(cipher_buffer, "histogram_words", lambda *a, **k: calls.append(1))
    with pytest.raises(OverflowError):
        src.histogram(np.zeros((N, 1), dtype=np.uint8), 1)
    assert not calls


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "flexpai.h")) as f:
        h = f.read()
    from flex.crypto.paillier import _native as N
    assert re.search(r"enum\s*\{\s*PAI_BIN_U8\s*=\s*0\s*,\s*PAI_BIN_U16\s*=\s*1\s*\}", h)
    assert re.search(r"#define\s+PAI_HIST_RUN\s+(\d+)", h).group(1) == str(N.HIST_RUN)
    for name in ("pai_histogram", "pai_histogram_dev"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h) and name in N.EXPORTED
    assert (N.PAI_BIN_U8, N.PAI_BIN_U16) == (0, 1)
