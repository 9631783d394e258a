"""Prefix sums and axis sums without a GPU: the Python-int fallbacks of parallel_ops.cumsum, CiphertextBuffer.cumsum /
.sum and PackedCiphertextBuffer.cumsum against the reference fixture (tests/golden/paillier_golden_cumsum.json) and the
``+`` chain, np.cumsum / np.sum on a PaillierArray against the plain object ndarray, the argument errors, the overflow
refusal, and the C ABI's declarations."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = [("axis0", 0, False), ("axis0_rev", 0, True), ("axis1", 1, False), ("axis1_rev", 1, True)]
EMPTY = -(1 << 31)


@pytest.fixture(scope="module")
def gcs():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_cumsum.json")) as f:
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


def matches(case, tag, flat):
    if tag in case:
        return [[hex(c), e] for c, e in flat] == case[tag]
    return [hashlib.sha256(f"{hex(c)}:{e}".encode()).hexdigest() for c, e in flat] == case[tag + "_sha256"]


def pairs(arr):
    return [(e.ciphertext(False), e.exponent) for e in np.asarray(arr).reshape(-1)]


def _buffer(pk, ms, exps=None, seed=3, shape=None):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    n, nsq = pk.n, pk.nsquare
    W = (2 * n.bit_length() + 31) // 32
    cts = [(1 + n * (int(m) % n)) % nsq * pow(O.golden_r(n, seed, i), n, nsq) % nsq for i, m in enumerate(ms)]
    return CiphertextBuffer(pk, _runtime.ints_to_words(cts, W), np.zeros(len(cts), dtype=np.int32) if exps is None
                            else np.array(exps, dtype=np.int32), shape=shape)


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", ["labels", "floats"])
def test_fallbacks_reproduce_the_fixture(golden, gcs, no_gpu, name):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.cipher_array import PaillierArray, materialize
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer, cumsum_words
    from flex.crypto.paillier.keypair import PaillierPublicKey
    n = int(golden["keys"]["1024"]["n"], 16)
    pub = PaillierPublicKey(n)
    case = gcs["cases"][name]
    words = _runtime.ints_to_words([int(h, 16) for h in case["c"]], (2 * n.bit_length() + 31) // 32)
    exps = np.array(case["e"], dtype=np.int32)
    enc = materialize(pub, words, exps, (3, 9), obfuscated=True)
    buf = CiphertextBuffer(pub, words, exps, shape=(3, 9))
    for tag, axis, rev in TAGS:
        arr = parallel_ops.cumsum(np.asarray(enc), axis, reverse=rev)
        assert isinstance(arr, PaillierArray) and arr.shape == (3, 9)
        assert matches(case, tag, pairs(arr)), (name, tag)
        assert not any(e._is_obfuscated() for e in arr.reshape(-1))
        got = buf.cumsum(axis, reverse=rev)
        assert got.shape == (3, 9) and not got.obfuscated.any()
        assert matches(case, tag, list(zip(_runtime.words_to_ints(got.words), got.exps.tolist()))), (name, tag)
        outer, L, inner = (1, 3, 9) if axis == 0 else (3, 9, 1)
        w2, e2 = cumsum_words(pub, words, exps, outer, L, inner, rev)
        assert np.array_equal(w2, got.words) and np.array_equal(e2, got.exps)
    # negative axes, and the PaillierArray method (numpy's own loop without a GPU) on the forward scans
    assert np.array_equal(buf.cumsum(-1).words, buf.cumsum(1).words) and np.array_equal(buf.cumsum(-2).words, buf.cumsum(0).words)
    for axis in (0, 1):
        assert matches(case, f"axis{axis}", pairs(enc.cumsum(axis))) and matches(case, f"axis{axis}", pairs(np.cumsum(enc, axis)))


def test_empty_entries_are_the_identity(pkg):
    """Exponent INT32_MIN with ciphertext 1 (an empty segment) is skipped by cumsum_words: leading, in the middle, trailing,
    a whole row; nothing entered yet gives ciphertext 1 with INT32_MIN."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import cumsum_words
    pk, _, key = pkg
    buf = _buffer(pk, range(1, 13), exps=[EMPTY, 2, EMPTY, 5, 1, EMPTY] + [EMPTY] * 6)
    cs = _runtime.words_to_ints(buf.words)
    for rev in (False, True):
        out, oe = cumsum_words(pk, buf.words, buf.exps, 2, 6, 1, rev)
        got = _runtime.words_to_ints(out)
        for r in range(2):
            for j in range(6):
                mem = [r * 6 + t for t in (range(j, 6) if rev else range(j + 1)) if buf.exps[r * 6 + t] != EMPTY]
                want = O.add_k([cs[i] for i in mem], [int(buf.exps[i]) for i in mem], key) if mem else (1, EMPTY)
                assert (got[r * 6 + j], int(oe[r * 6 + j])) == want, (rev, r, j)


# ---------------------------------------------------------------- sums
def test_sum_equals_the_add_chain(pkg):
    from flex.crypto.paillier import _runtime
    pk, _, _ = pkg
    rng = np.random.default_rng(11)
    buf = _buffer(pk, rng.integers(-50, 50, 24), exps=rng.integers(0, 4, 24), shape=(2, 3, 4))
    arr = buf.to_array()
    plain = np.asarray(arr).view(np.ndarray)
    for axis in (0, 1, 2, -1):
        got = buf.sum(axis)
        want = plain.sum(axis=axis)                            # numpy's object reduction: the + chain
        assert got.shape == want.shape and not got.obfuscated.any()
        assert list(zip(_runtime.words_to_ints(got.words), got.exps.tolist())) == pairs(want), axis
    total = buf.sum()
    assert total.shape == (1,)
    t = plain.sum()
    assert (_runtime.words_to_ints(total.words)[0], int(total.exps[0])) == (t.ciphertext(False), t.exponent)
    # an empty reduction: the unobfuscated encryption of 0
    e = _buffer(pk, [], shape=(0, 3)).sum(0)
    assert e.shape == (3,) and _runtime.words_to_ints(e.words) == [1, 1, 1] and e.exps.tolist() == [0, 0, 0]


def test_numpy_entry_points_match_the_plain_object_array(pkg, monkeypatch):
    """Without a GPU the overrides hand over to numpy's own loop; the GPU side of the same comparison is
    test_gpu_cumsum.py::test_sums_and_numpy_entry_points. Here: the overrides exist, np.cumsum / np.sum reach them, and
    they ask cumsum_encrypted / sum_encrypted first."""
    from flex.crypto.paillier import cipher_array
    from flex.crypto.paillier.cipher_array import PaillierArray
    pk, _, _ = pkg
    assert PaillierArray.cumsum is not np.ndarray.cumsum and PaillierArray.sum is not np.ndarray.sum
    asked = []
    real_c, real_s = cipher_array.cumsum_encrypted, cipher_array.sum_encrypted
    monkeypatch.setattr(cipher_array, "cumsum_encrypted", lambda a, axis=None, **k: asked.append(("cumsum", axis)) or real_c(a, axis, **k))
    monkeypatch.setattr(cipher_array, "sum_encrypted", lambda a, axis=None: asked.append(("sum", axis)) or real_s(a, axis))
    rng = np.random.default_rng(12)
    arr = _buffer(pk, rng.integers(-9, 9, 12), exps=rng.integers(0, 3, 12), shape=(3, 4)).to_array()
    assert isinstance(arr, PaillierArray)
    plain = np.asarray(arr).view(np.ndarray)
    for axis in (None, 0, 1, -1):
        for got in (np.cumsum(arr, axis), arr.cumsum(axis), arr.cumsum(axis=axis)):
            want = np.cumsum(plain, axis)
            assert got.shape == want.shape and pairs(got) == pairs(want), axis
        for got in (np.sum(arr, axis), arr.sum(axis), arr.sum(axis=axis)):
            want = np.sum(plain, axis)
            assert np.shape(got) == np.shape(want) and pairs(got) == pairs(want), axis
    assert asked.count(("cumsum", 0)) == 3 and asked.count(("sum", None)) == 3 and len(asked) == 24
    # dtype= or out= go to numpy without asking
    arr.cumsum(0, dtype=object)
    assert len(asked) == 24
    # anything else inside: numpy's own loop, unchanged
    mixed = PaillierArray(np.array([arr[0, 0], 3, arr[0, 1]], dtype=object))
    got = np.cumsum(mixed)
    want = np.cumsum(np.array([arr[0, 0], 3, arr[0, 1]], dtype=object))
    assert [(e.ciphertext(False), e.exponent) for e in got] == [(e.ciphertext(False), e.exponent) for e in want]
    assert np.cumsum(PaillierArray(np.array([1, 2, 3], dtype=object))).tolist() == [1, 3, 6]


# ---------------------------------------------------------------- packed
def test_packed_cumsum_and_the_overflow_refusal(pkg, monkeypatch):
    from flex.crypto.paillier import cipher_buffer
    from flex.crypto.paillier.packed_buffer import (PackedCiphertextBuffer, PackedLayout, host_decrypt_packed,
                                                    host_encrypt_packed)
    pk, sk, _ = pkg
    lay = PackedLayout(pk, 32, 11, 0, 2)
    rng = np.random.default_rng(13)
    gh = rng.integers(-1000, 1001, (2, 3, 4, 2)).astype(np.int64)
    words, st = host_encrypt_packed(gh.reshape(-1), lay, pk)
    assert not st.any()
    src = PackedCiphertextBuffer(pk, words, lay, gh.size, gh.shape, False, 1000)
    for axis, rev in ((2, False), (0, False), (1, True), (-1, False)):
        out = src.cumsum(axis, reverse=rev)
        ax = axis % 3
        want = np.flip(np.cumsum(np.flip(gh, ax), ax), ax) if rev else np.cumsum(gh, ax)
        assert out.shape == gh.shape and out.bound == 1000 * gh.shape[ax] and not out.obfuscated
        assert host_decrypt_packed(out, sk) == want.reshape(-1).tolist(), (axis, rev)
    # the slot axis, a buffer that is not (..., slots), a ragged last ciphertext
    with pytest.raises(ValueError):
        src.cumsum(3)
    with pytest.raises(ValueError):
        PackedCiphertextBuffer(pk, words, lay, gh.size, (gh.size,), False, 1000).cumsum(0)
    with pytest.raises(ValueError):
        PackedCiphertextBuffer(pk, words, lay, gh.size, (12, 4), False, 1000).cumsum(0)
    # the refusal fires before any product
    calls = []
    monkeypatch.setattr(cipher_buffer, "cumsum_words", lambda *a, **k: calls.append(1))
    src.bound = lay.slot_max // 3
    with pytest.raises(OverflowError):
        src.cumsum(2)
    assert not calls


# ---------------------------------------------------------------- arguments, declarations
def test_argument_errors(pkg):
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.cipher_buffer import axis_split, cumsum_words
    pk, _, _ = pkg
    buf = _buffer(pk, range(6), shape=(2, 3))
    assert axis_split((2, 3, 4), 1) == (2, 3, 4) and axis_split((2, 3, 4), -1) == (6, 4, 1) and axis_split((5,), 0) == (1, 5, 1)
    for bad in (2, -3):
        with pytest.raises(ValueError):
            buf.cumsum(bad)
        with pytest.raises(ValueError):
            buf.sum(bad)
    with pytest.raises(TypeError):
        buf.cumsum(1.0)
    with pytest.raises(TypeError):
        buf.cumsum(True)
    with pytest.raises(ValueError):
        cumsum_words(pk, buf.words, buf.exps, 2, 2, 1)
    with pytest.raises(TypeError):
        parallel_ops.cumsum([1, 2, 3])
    with pytest.raises(TypeError):
        parallel_ops.cumsum(np.array([1, 2, 3], dtype=object))
    with pytest.raises(ValueError):
        parallel_ops.cumsum(np.asarray(buf.to_array()), 2)


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "flexpai.h")) as f:
        h = f.read()
    assert re.search(r"int pai_cumsum\(pai_ctx\* ctx, const uint32_t\* ct, const int32_t\* exp, size_t outer, size_t L, "
                     r"size_t inner,\s+int flags,\s+uint32_t\* ct_out, int32_t\* exp_out\);", h)
    assert re.search(r"int pai_cumsum_dev\(pai_ctx\* ctx, const uint32_t\* d_ct, const int32_t\* d_exp, size_t outer, size_t L, "
                     r"size_t inner,\s+int flags, uint32_t\* d_out, int32_t\* d_exp_out, void\* stream\);", h)
    assert "PAI_SCAN_REVERSE = 1" in h and re.search(r"#define PAI_OPT_SCAN_TILE 23\b", h) and re.search(r"#define PAI_OPT_SCAN_PATH 24\b", h)
    from flex.crypto.paillier import _native
    assert "pai_cumsum" in _native.EXPORTED and "pai_cumsum_dev" in _native.EXPORTED
    assert (_native.PAI_OPT_SCAN_TILE, _native.PAI_OPT_SCAN_PATH, _native.PAI_SCAN_REVERSE) == (23, 24, 1)
