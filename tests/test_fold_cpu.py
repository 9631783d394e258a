"""pai_pack_ciphertexts without a GPU: the reference fixture (tests/golden/paillier_golden_fold.json) against the CPU
oracle and the Python-int fallback of the package (packed_buffer.host_pack_ciphertexts, pack_ciphertexts,
parallel_ops.segment_sum_packed), the bound arithmetic, the errors, and the C ABI's declarations."""
import json
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1024, 2048, 4096)
EMPTY = -(1 << 31)


def unpack(m, n, sb, k):
    max_int = n // 3 - 1
    if m <= max_int:
        M = m
    elif m >= n - max_int:
        M = m - n
    else:
        return None
    B, out = 1 << sb, []
    for _ in range(k):
        t = ((M + B // 2) % B) - B // 2
        out.append(t)
        M = (M - t) // B
    return out if M == 0 else None


def mul_pow2(c, e, bits, key):
    """c * 2^bits through oracle.mul_scalar, whose encoder takes scalars below the float range: factors of at most
    2^960 in turn (pow(pow(c, 2^a), 2^b) = pow(c, 2^(a + b)) mod n^2)."""
    c, e = O.mul_scalar(c, e, 1 << (bits % 960), key)
    for _ in range(bits // 960):
        c, e = O.mul_scalar(c, e, 1 << 960, key)
    return c, e


@pytest.fixture(scope="module")
def golden_fold():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_fold.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pkg():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=5)
    mp = pytest.MonkeyPatch()
    mp.setattr(_runtime, "gpu_available", lambda: False)       # the Python-int fallback, wherever the suite runs
    yield pk, sk, PaillierDecryptor(pk, sk)
    mp.undo()


def _buffer(pk, ms, exps, seed=1):
    """A CiphertextBuffer of the integers ms held at the exponents exps (value m 16^-e), obfuscated, no GPU."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    n, nsq = pk.n, pk.nsquare
    W = (2 * n.bit_length() + 31) // 32
    cts = [(1 + n * (m % n)) % nsq * pow(O.golden_r(n, seed, i), n, nsq) % nsq for i, m in enumerate(ms)]
    return CiphertextBuffer(pk, _runtime.ints_to_words(cts, W), np.array(exps, dtype=np.int32)), cts


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("nb", NBS)
def test_fixture_and_host_fallback(golden, golden_fold, nb):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_pack_ciphertexts
    kk = golden["keys"][str(nb)]
    key = O.Key(int(kk["n"], 16), int(kk["p"], 16), int(kk["q"], 16))
    n, nsq = key.n, key.nsquare
    rec = golden_fold["cases"][str(nb)]
    sb, E, k = rec["slot_bits"], rec["exponent"], rec["slots"]
    ts, ds = rec["t"], rec["delta"]
    cts = [int(h, 16) for h in rec["ct"]]
    assert len(ts) == len(ds) == len(cts) == 2 * k + 1 and set(ds) == {0, 1, 2} and k <= (nb - 2) // sb
    assert ds[0] == ds[k] == ds[2 * k] == 0 and ds[k - 1] == 2 and ds[2 * k - 1] == 1
    for i in (0, k - 1, 2 * k):                                # the inputs are the reference's raw_encrypt under golden_r
        assert cts[i] == O.raw_encrypt(ts[i] % n, key, O.golden_r(n, 900, i)), (nb, i)
    # the fallback against the reference's folded ciphertexts
    lay = PackedLayout(PaillierPublicKey(n), sb, sb, E, k)
    got, st = host_pack_ciphertexts(cts, [E - d for d in ds], lay, PaillierPublicKey(n))
    assert [hex(c) for c in got] == rec["folded"] and not st.any() and st.dtype == np.int32
    # ... and the integer definition, through the oracle's operators, on the ragged last output and the first one
    last = O.mul_scalar(cts[2 * k], E - ds[2 * k], 1, key)
    assert (int(rec["folded"][2], 16), E) == last
    terms = [mul_pow2(c, E - d, sb * j, key) for j, (c, d) in enumerate(zip(cts[:k], ds[:k]))]
    assert (int(rec["folded"][0], 16), E) == O.add_k([t[0] for t in terms], [t[1] for t in terms], key)
    # the raw plaintexts decode to the slot integers t 16^D
    want = [t << (4 * d) for t, d in zip(ts, ds)]
    raws = [int(h, 16) for h in rec["raw"]]
    assert [v for m in raws for v in unpack(m, n, sb, k)][:len(want)] == want
    assert O.raw_decrypt(int(rec["folded"][1], 16), key) == raws[1]
    assert golden_fold["gmpy2"] and golden_fold["generator"].endswith("make_golden_fold.py")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "paillier_golden_fold.json")) < 300 * 1024


def test_host_fallback_against_the_integer_definition(pkg):
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_pack_ciphertexts
    pk, sk, dec = pkg
    n, nsq = pk.n, pk.nsquare
    lay = PackedLayout(pk, 32, 32, 4, 5)
    sb, E, k = 32, 4, 5
    ms = [7, -9, 3, -1, 5, 6, -7, 8, 9, -10, 11, 12]
    exps = [4, 3, E - 7, 5, EMPTY, 4, E - 8, 2, 4, (1 << 31) - 1, -(1 << 31) + 1, 4]
    buf, cts = _buffer(pk, ms, exps)
    got, st = host_pack_ciphertexts(cts, exps, lay, pk)
    assert st.tolist() == [0, 0, 0, 5, 0, 0, 5, 0, 0, 5, 5, 0]
    want = [1, 1, 1]
    for i, (c, e) in enumerate(zip(cts, exps)):
        if st[i] == 0 and e != EMPTY:
            want[i // k] = want[i // k] * pow(c, 1 << (4 * (E - e) + sb * (i % k)), nsq) % nsq
    assert got == want
    slots = [m << (4 * (E - e)) if s == 0 and e != EMPTY else 0 for m, e, s in zip(ms, exps, st)]
    raw = [O.raw_decrypt(c, O.Key(n, sk.p, sk.q)) for c in got]
    assert [v for m in raw for v in unpack(m, n, sb, k)][:len(ms)] == slots
    # (1 + n m)^e = 1 + n m e mod n^2: the closed form the GPU tests use for unobfuscated inputs
    c0 = [(1 + n * (m % n)) % nsq for m in ms]
    got0, _ = host_pack_ciphertexts(c0, exps, lay, pk)
    assert got0 == [(1 + n * (sum(t << (sb * j) for j, t in enumerate(slots[c:c + k])) % n)) % nsq for c in (0, 5, 10)]
    assert host_pack_ciphertexts([], [], lay, pk)[0] == []


# ---------------------------------------------------------------- the package on Python integers
def test_pack_ciphertexts_fallback_round_trip(pkg):
    from flex.crypto.paillier.cipher_array import PaillierArray
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout, add_packed, pack_ciphertexts
    pk, sk, dec = pkg
    lay = PackedLayout(pk, 32, 32, 2)
    assert lay.slots == 31
    rng = np.random.default_rng(4)
    ms = [int(v) for v in rng.integers(-4000, 4001, 40)]       # 40 values: two ciphertexts, the second ragged
    exps = [2 - int(d) for d in rng.integers(0, 3, 40)]
    buf, cts = _buffer(pk, ms, exps)
    buf = buf.reshape(5, 8)
    packed = pack_ciphertexts(buf, lay, 4000)                  # |value| = |m| 16^-e <= 4000: the caller's assertion
    assert isinstance(packed, PackedCiphertextBuffer) and packed.words.shape == (2, 64) and packed.shape == (5, 8)
    assert packed.count == 40 and packed.bound == 4000 * 256 and not packed.obfuscated and packed.layout == lay
    want = np.array([m << (4 * (2 - e)) for m, e in zip(ms, exps)], dtype=np.float64).reshape(5, 8) * 16.0 ** -2
    assert np.array_equal(dec.decrypt(packed), want)
    assert np.array_equal(buf.pack(lay, 4000).words, packed.words), "deterministic: not re-randomised"
    # an object array and a PaillierArray give the same bits
    objs = np.empty(40, dtype=object)
    objs[:] = [PaillierEncryptedNumber(pk, c, e) for c, e in zip(cts, exps)]
    assert np.array_equal(pack_ciphertexts(objs.reshape(5, 8), lay, 4000).words, packed.words)
    arr = PaillierArray(objs.reshape(5, 8))
    assert np.array_equal(arr.pack(lay, 4000).words, packed.words) and arr.pack(lay, 4000).shape == (5, 8)
    # the result is an ordinary packed buffer: sums, integer products, the wire
    before = packed.words.copy()
    back = PackedCiphertextBuffer.from_wire(add_packed([packed, packed * -3]).to_wire(be_secure=True), pk)
    assert back.obfuscated and back.bound == 4 * 4000 * 256 and np.array_equal(dec.decrypt(back), -2 * want)
    assert np.array_equal(packed.words, before)


def test_bounds_are_refused_before_any_native_call(pkg, monkeypatch):
    from flex.crypto.paillier import _runtime, packed_buffer
    from flex.crypto.paillier.packed_buffer import PackedLayout, pack_ciphertexts
    from flex.crypto.paillier.parallel_ops import segment_sum_packed
    pk, sk, dec = pkg
    buf, _ = _buffer(pk, [1, 2, 3, 4], [0, 0, 0, 0])

    def boom(*a, **kw):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_runtime, "context", boom)
    monkeypatch.setattr(_runtime, "gpu_available", boom)
    monkeypatch.setattr(packed_buffer, "_ints", boom)
    monkeypatch.setattr(packed_buffer, "_gpu", boom)
    lay = PackedLayout(pk, 16, 16, 2)                          # slot_max = 32767, 16^2 = 256
    for max_abs in (128, 127.997, 1 << 40):                    # ceil(max_abs 256) > 32767
        with pytest.raises(OverflowError):
            pack_ciphertexts(buf, lay, max_abs)
        with pytest.raises(OverflowError):
            buf.pack(lay, max_abs)
    with pytest.raises(OverflowError):
        segment_sum_packed(buf, [[0, 1, 2], [3]], lay, 43)     # 3 * ceil(43 * 256) = 33024
    with pytest.raises(AssertionError, match="native call"):
        pack_ciphertexts(buf, lay, 127.99)                     # ceil(127.99 * 256) = 32766: goes on to the fold
    with pytest.raises(AssertionError, match="native call"):
        segment_sum_packed(buf, [[0, 1, 2], [3]], lay, 42)     # 3 * 10752 = 32256


def test_bound_arithmetic(pkg):
    from flex.crypto.paillier.packed_buffer import PackedLayout, pack_ciphertexts
    from flex.crypto.paillier.parallel_ops import segment_sum_packed
    pk, sk, dec = pkg
    buf, _ = _buffer(pk, [1, 0, 1, 1, 0, 1], [0] * 6)
    for max_abs, e, bound in ((1, 0, 1), (2.5, 1, 40), (0.01, 2, 3), (127.99, 2, 32766)):
        assert pack_ciphertexts(buf, PackedLayout(pk, 16, 16, e), max_abs).bound == bound
    lay = PackedLayout(pk, 16, 16, 0)
    packed = segment_sum_packed(buf, [[0, 2, 3, 5], [], [1], [4, 0]], lay, 1)
    assert packed.bound == 4 and packed.count == 4 and packed.shape == (4,) and not packed.obfuscated
    got = dec.decrypt(packed)
    assert got.dtype == np.int64 and got.tolist() == [4, 0, 0, 1]      # the empty bin decodes as 0
    assert dec.decrypt(segment_sum_packed(buf, [[-1, -6]], lay, 1)).tolist() == [2]     # numpy's negative indices
    assert segment_sum_packed(buf, [[], []], lay, 1).bound == 0
    # members of one bin at different exponents are aligned to the bin's largest, as pai_segment_add does
    mixed, _ = _buffer(pk, [3, 5, 7], [1, 0, 1])
    assert dec.decrypt(segment_sum_packed(mixed, [[0, 1], [2]], PackedLayout(pk, 16, 16, 1), 8)).tolist() == [
        (3 + 5 * 16) / 16, 7 / 16]


def test_errors(pkg):
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, pack_ciphertexts
    from flex.crypto.paillier.parallel_ops import segment_sum_packed
    pk, sk, dec = pkg
    lay = PackedLayout(pk, 32, 32, 0)
    buf, cts = _buffer(pk, list(range(9)), [0, 0, -1, -7, -8, 0, 1, 0, 0])
    with pytest.raises(ValueError, match="index 4"):           # 4 D = 32 is the first exponent out of range
        pack_ciphertexts(buf, lay, 1)
    ok = CiphertextBuffer(pk, buf.words, np.array([0, 0, -1, -7, 0, 0, 1, 0, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="index 6"):           # an exponent above the layout's
        ok.pack(lay, 1)
    for src in (np.arange(4), [1, 2], 3.0, None, np.array([1, "a"], dtype=object), np.array([], dtype=object)):
        with pytest.raises(TypeError):
            pack_ciphertexts(src, lay, 1)
    with pytest.raises(TypeError):
        segment_sum_packed(np.arange(4), [[0]], lay, 1)
    pk2 = PaillierPublicKey((1 << 2047) + 9)                    # a key of another size
    with pytest.raises(ValueError, match="layout does not belong"):
        pack_ciphertexts(buf, PackedLayout(pk2, 32, 32, 0), 1)
    with pytest.raises(ValueError, match="layout does not belong"):
        pack_ciphertexts(buf, (32, 32, 0, 31), 1)
    with pytest.raises(ValueError, match="layout does not belong"):
        segment_sum_packed(buf, [[0]], (32, 32, 0, 31), 1)
    # a result under one key does not add to one under another key of the same size
    other = PaillierPublicKey(pk.n + 2)
    a = pack_ciphertexts(CiphertextBuffer(pk, buf.words[:2], np.zeros(2, dtype=np.int32)), lay, 1)
    b = pack_ciphertexts(CiphertextBuffer(other, buf.words[:2], np.zeros(2, dtype=np.int32)),
                         PackedLayout(other, 32, 32, 0), 1)
    with pytest.raises(ValueError, match="public key"):
        a + b


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_symbols():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flexpai.h")).read())
    assert ("int pai_pack_ciphertexts(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, "
            "const pai_pack_layout* layout, uint32_t* ct_out, int32_t* status_out);") in header
    assert ("int pai_pack_ciphertexts_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, "
            "const pai_pack_layout* layout, uint32_t* d_out, int32_t* d_status, void* stream);") in header
    assert not re.search(r"#define PAI_OPT_\w+ 19\b", header) and not re.search(r"#define PAI_EL_\w+ 6\b", header)
    from flex.crypto.paillier import _native
    names = {"pai_pack_ciphertexts", "pai_pack_ciphertexts_dev"}
    assert names <= set(_native.EXPORTED)
    lib = _native.load_library()
    assert len(lib.pai_pack_ciphertexts.argtypes) == 7 and len(lib.pai_pack_ciphertexts_dev.argtypes) == 8
    for name in names:
        assert getattr(lib, name).restype is not None
    assert callable(_native.Context.pack_ciphertexts)
