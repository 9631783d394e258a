"""Packed plaintexts without a GPU: the reference fixture (tests/golden/paillier_golden_packed.json) against the CPU
oracle and the pack / unpack definitions of include/flexpai.h, the layout rules, the bound arithmetic, the wire format,
the Python-int fallback of the package, and the C ABI's declarations."""
import json
import math
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1024, 2048, 4096)


def pack(ts, sb):
    return sum(int(t) << (sb * j) for j, t in enumerate(ts))


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


@pytest.fixture(scope="module")
def golden_packed():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_packed.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pkg():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=5)
    mp = pytest.MonkeyPatch()
    mp.setattr(_runtime, "gpu_available", lambda: False)       # the Python-int fallback, wherever the suite runs
    yield pk, sk, PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    mp.undo()


@pytest.fixture(scope="module")
def pk1024(golden):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    return PaillierPublicKey(int(golden["keys"]["1024"]["n"], 16))


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("nb", NBS)
def test_fixture_reproduces_from_oracle(golden, golden_packed, nb):
    k = golden["keys"][str(nb)]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    n, nsq = key.n, key.nsquare
    recs = golden_packed["cases"][str(nb)]
    assert len(recs) == 2
    for li, rec in enumerate(recs):
        sb, vb, e, slots = rec["slot_bits"], rec["value_bits"], rec["exponent"], rec["slots"]
        assert slots == (nb - 2) // sb and sb % 8 == 0 and 2 <= vb <= sb and len(rec["t"]) == 3
        mx = (1 << (vb - 1)) - 1
        assert rec["t"][1] == [-mx] * slots and rec["t"][2][:2] == [mx, -mx]
        cts = [int(h, 16) for h in rec["ct"]]
        for i, (ts, r, c, raw) in enumerate(zip(rec["t"], rec["r"], cts, rec["raw"])):
            assert len(ts) == slots and all(abs(t) <= mx for t in ts)
            M = pack(ts, sb)
            assert abs(M) < 1 << (slots * sb - 1) <= 1 << (nb - 3) < key.max_int
            assert r == hex(O.golden_r(n, 800 + li, i))
            if i == 0 or nb < 4096:
                assert c == O.raw_encrypt(M % n, key, int(r, 16)), (nb, li, i)
                assert O.raw_decrypt(c, key) == int(raw, 16)
            assert int(raw, 16) == M % n and unpack(int(raw, 16), n, sb, slots) == ts
        assert int(rec["sum3"], 16) == cts[0] * cts[1] * cts[2] % nsq
        assert int(rec["mul_m3"], 16) == O.mul_scalar(cts[0], e, -3, key)[0]
        assert unpack(int(rec["raw_sum3"], 16), n, sb, slots) == [a + b + c for a, b, c in zip(*rec["t"])]
        assert unpack(int(rec["raw_mul_m3"], 16), n, sb, slots) == [-3 * a for a in rec["t"][0]]
    assert golden_packed["gmpy2"] and golden_packed["generator"].endswith("make_golden_packed.py")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "paillier_golden_packed.json")) < 300 * 1024


# ---------------------------------------------------------------- layouts
def test_layout_validation_and_for_sum(golden, pk1024):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout
    for nb in NBS:                                             # the most slots keep |M| below max_int
        pk = PaillierPublicKey(int(golden["keys"][str(nb)]["n"], 16))
        for sb in range(16, 65, 8):
            k = PackedLayout(pk, sb, sb, 0).slots
            assert k == (nb - 2) // sb and 1 << (k * sb - 1) <= 1 << (nb - 3) < pk.max_int
    lay = PackedLayout(pk1024, 32, 24, 5)
    assert lay.as_tuple() == (32, 24, 5, 31) and lay.value_max == (1 << 23) - 1 and lay.slot_max == (1 << 31) - 1
    assert PackedLayout(pk1024, 64, 64, 0, 3).slots == 3 and PackedLayout(pk1024, 16, 2, -1).slots == 63
    assert lay == PackedLayout(pk1024, 32, 24, 5, 31) and lay != PackedLayout(pk1024, 32, 24, 5, 30)
    for bad in ((20, 16, 0, None), (8, 8, 0, None), (72, 64, 0, None), (32, 33, 0, None), (32, 1, 0, None),
                (32, 24, 0, 32), (32, 24, 0, 0)):
        with pytest.raises(ValueError):
            PackedLayout(pk1024, *bad)
    assert PackedLayout.for_sum(pk1024, 4.0, 5, terms=2).as_tuple() == (32, 24, 5, 31)     # 4 * 16^5 = 2^22
    assert PackedLayout.for_sum(pk1024, 4.0, 5, terms=256).as_tuple() == (32, 24, 5, 31)
    assert PackedLayout.for_sum(pk1024, 4.0, 5, terms=257).as_tuple() == (40, 24, 5, 25)
    assert PackedLayout.for_sum(pk1024, 3.99, 5).as_tuple()[:2] == (24, 23)
    assert PackedLayout.for_sum(pk1024, 60.0, 6, terms=2).as_tuple()[:2] == (32, 31)
    assert PackedLayout.for_sum(pk1024, 1, 0).as_tuple()[:2] == (16, 2)
    assert PackedLayout.for_sum(pk1024, 1.0, 13, terms=1024).as_tuple()[:2] == (64, 54)
    with pytest.raises(ValueError):
        PackedLayout.for_sum(pk1024, 1.0, 13, terms=2048)
    # for_sum's promise: `terms` values at max_abs never pass the slot
    for max_abs, e, terms in ((4.0, 5, 2), (4.0, 5, 256), (0.1, 7, 3), (1234.5, 3, 9)):
        lay = PackedLayout.for_sum(pk1024, max_abs, e, terms)
        t = round(math.ldexp(max_abs, 4 * e))
        assert t <= lay.value_max and terms * lay.value_max <= lay.slot_max


# ---------------------------------------------------------------- bounds: refused before any native call
def _buffers(pk, layout, count=40, nbuf=2):
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer
    W = (2 * pk.n.bit_length() + 31) // 32
    C = -(-count // layout.slots)
    words = np.zeros((C, W), dtype=np.uint32)
    words[:, 0] = 1                                            # the ciphertext 1: every slot 0
    return [PackedCiphertextBuffer(pk, words.copy(), layout, count) for _ in range(nbuf)]


def test_bound_arithmetic_refuses_before_any_native_call(pk1024, monkeypatch):
    from flex.crypto.paillier import _runtime, packed_buffer
    from flex.crypto.paillier.packed_buffer import PackedLayout, add_packed

    def boom(*a, **kw):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_runtime, "context", boom)
    monkeypatch.setattr(_runtime, "gpu_available", boom)
    monkeypatch.setattr(packed_buffer, "_ints", boom)
    lay = PackedLayout(pk1024, 32, 31, 4)
    a, b = _buffers(pk1024, lay)
    assert a.bound == (1 << 30) - 1
    a.bound = b.bound = (1 << 30)                              # 2^30 + 2^30 = 2^31 > 2^31 - 1
    for op in (lambda: a + b, lambda: a - b, lambda: add_packed([a, b]), lambda: a * 2, lambda: a * -2, lambda: 2 * a,
               lambda: a * np.int64(3), lambda: a * ((1 << 63) - 1)):
        with pytest.raises(OverflowError):
            op()
    with pytest.raises(OverflowError):
        a * (1 << 63)
    for s in (0.5, np.float32(2.0), "2", None, True):
        with pytest.raises(TypeError):
            a * s
    with pytest.raises(TypeError):
        a + 1
    other_lay, = _buffers(pk1024, PackedLayout(pk1024, 32, 30, 4), nbuf=1)
    with pytest.raises(ValueError, match="layouts differ"):
        a + other_lay
    from flex.crypto.paillier.keypair import PaillierPublicKey
    other_key, = _buffers(PaillierPublicKey(pk1024.n + 2), lay, nbuf=1)
    with pytest.raises(ValueError, match="public key"):
        a + other_key
    with pytest.raises(ValueError, match="shapes"):
        a + _buffers(pk1024, lay, count=41, nbuf=1)[0]
    with pytest.raises(OverflowError):
        _buffers(pk1024, lay, nbuf=1)[0].__class__(pk1024, a.words, lay, 40, bound=1 << 31)


def test_bounds_follow_the_operations(pkg):
    from flex.crypto.paillier.packed_buffer import PackedLayout, add_packed
    pk, sk, enc, dec = pkg
    lay = PackedLayout(pk, 32, 20, 0)
    a, b = _buffers(pk, lay)
    v = lay.value_max
    assert (a + b).bound == 2 * v and (a - b).bound == 2 * v and add_packed([a, b, a]).bound == 3 * v
    assert (a * -5).bound == 5 * v and (a * 0).bound == 0 and ((a + b) * 3).bound == 6 * v
    assert add_packed([a]) is a and not (a + b).obfuscated


# ---------------------------------------------------------------- wire
def test_wire_round_trip_and_malformed_bytes(pk1024):
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    lay = PackedLayout(pk1024, 32, 24, 5)
    W = 64
    rng = np.random.default_rng(3)
    words = rng.integers(0, 1 << 32, (3, W), dtype=np.uint64).astype(np.uint32)
    words[:, -1] = 0                                           # below n^2
    buf = PackedCiphertextBuffer(pk1024, words, lay, 70, (7, 10), obfuscated=True, bound=1234567890)
    wire = buf.to_wire()
    assert len(wire) < 3 * 4 * W + 250
    for key in (None, pk1024):
        back = PackedCiphertextBuffer.from_wire(wire, key)
        assert np.array_equal(back.words, words) and back.layout == lay and back.count == 70 and back.shape == (7, 10)
        assert back.obfuscated is True and back.bound == 1234567890 and back.public_key == pk1024
    plain = PackedCiphertextBuffer(pk1024, words, lay, 70)
    assert PackedCiphertextBuffer.from_wire(plain.to_wire()).obfuscated is False
    assert PackedCiphertextBuffer.from_wire(plain.to_wire()).bound == lay.value_max
    from flex.crypto.paillier.cipher_array import from_wire as array_from_wire
    from flex.crypto.paillier.keypair import PaillierPublicKey
    with pytest.raises(ValueError):
        array_from_wire(wire)                                  # its own magic: not a ciphertext array
    with pytest.raises(ValueError, match="different public key"):
        PackedCiphertextBuffer.from_wire(wire, PaillierPublicKey(pk1024.n + 2))
    head = len(wire) - 3 * 4 * W

    def patched(offset, data):
        b = bytearray(wire)
        b[offset:offset + len(data)] = data
        return bytes(b)
    o_n = 6 + 4
    o_w = o_n + 128
    o_lay = o_w + 4
    o_count = o_lay + 16
    o_shape = o_count + 8 + 4
    o_bound = o_shape + 16 + 4
    assert o_bound + 4 + 1 == head
    big = (pk1024.n * pk1024.n).to_bytes(4 * W, "little")
    for bad in (b"", wire[:5], b"XXXXX\0" + wire[6:], wire[:-4], wire + b"\0\0\0\0", wire[:head - 3],
                patched(o_w, np.uint32(63).tobytes()),                       # a wrong W
                patched(o_lay, np.int32(20).tobytes()),                      # slot_bits 20
                patched(o_lay + 4, np.int32(33).tobytes()),                  # value_bits > slot_bits
                patched(o_lay + 12, np.int32(32).tobytes()),                 # slots above the maximum
                patched(o_lay + 12, np.int32(23).tobytes()),                 # 70 values need 4 ciphertexts of 23
                patched(o_count, np.uint64(94).tobytes()),                   # count above C * slots
                patched(o_count, np.uint64(62).tobytes()),                   # ... and one that needs only 2
                patched(o_shape, np.int64(8).tobytes()),                     # shape does not match count
                patched(o_shape, np.int64(-7).tobytes()),
                patched(o_bound, (1 << 31).to_bytes(4, "little")),           # bound above the slot
                patched(head - 1, b"\x02"),                                  # unknown flag
                patched(head + 4 * W, big)):                                 # a word row = n^2
        with pytest.raises(ValueError):
            PackedCiphertextBuffer.from_wire(bad)


# ---------------------------------------------------------------- the Python-int fallback
def test_host_fallback_round_trip(pkg):
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, sk, enc, dec = pkg
    e = 5
    lay = PackedLayout.for_sum(pk, 4.0, e, terms=4)
    assert lay.as_tuple() == (32, 24, 5, 31)
    rng = np.random.default_rng(9)
    a = rng.uniform(-4, 4, (5, 8)).astype(np.float32)          # 40 values: 2 ciphertexts, the second ragged
    b = rng.uniform(-4, 4, (5, 8)).astype(np.float32)
    a[0, 0], a[0, 1], a[0, 2] = 4.0, -4.0, -0.0
    ta = np.array([round(math.ldexp(float(v), 4 * e)) for v in a.reshape(-1)])
    tb = np.array([round(math.ldexp(float(v), 4 * e)) for v in b.reshape(-1)])
    ea, eb = enc.encrypt_packed(a, lay), enc.encrypt_packed(b, lay)
    assert ea.words.shape == (2, 64) and ea.obfuscated and ea.bound == lay.value_max and ea.shape == (5, 8)
    assert np.array_equal(dec.decrypt(ea), ta.reshape(5, 8) * 16.0 ** -e)
    total = (ea + eb) * -2
    assert total.bound == 4 * lay.value_max and not total.obfuscated
    before = total.words.copy()
    back = PackedCiphertextBuffer.from_wire(total.to_wire(be_secure=True), pk)
    assert back.obfuscated and total.obfuscated and (back.words != before).any(axis=1).all()
    got = dec.decrypt(back)
    assert got.dtype == np.float64 and np.array_equal(got, (-2 * (ta + tb)).reshape(5, 8) * 16.0 ** -e)
    assert np.array_equal(dec.decrypt(ea - eb), (ta - tb).reshape(5, 8) * 16.0 ** -e)
    assert lay.slot_max // lay.value_max == 256
    with pytest.raises(OverflowError):
        total * 65                                             # 4 * 65 = 260 values' worth: past the slot
    # integers at exponent 0 come back as int64
    ilay = PackedLayout(pk, 64, 64, 0)
    x = np.array([(1 << 63) - 1, -(1 << 63) + 1, 0, -1, 7], dtype=np.int64)
    got = dec.decrypt(enc.encrypt_packed(x, ilay))
    assert got.dtype == np.int64 and np.array_equal(got, x)
    with pytest.raises(ValueError, match="index 1"):
        enc.encrypt_packed(np.array([1, -(1 << 63)], dtype=np.int64), ilay)
    with pytest.raises(ValueError, match="index 2"):
        enc.encrypt_packed(np.array([0.0, 4.0, 8.0, np.nan]), lay)
    with pytest.raises(TypeError):
        enc.encrypt_packed(np.array(["a"]), lay)
    # a plaintext in the gap raises the reference's OverflowError
    gap = PackedCiphertextBuffer(pk, _words_of((1 + pk.n * (pk.n // 2)) % pk.nsquare, 64), lay, 31)
    with pytest.raises(OverflowError, match="Overflow detected in decode number"):
        dec.decrypt(gap)


def _words_of(c, W):
    return np.frombuffer(c.to_bytes(4 * W, "little"), dtype="<u4").reshape(1, W).copy()


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_symbols():
    header = open(os.path.join(ROOT, "include", "flexpai.h")).read()
    declared = set(re.findall(r"^\s*int\s+(pai_\w+)\s*\(", header, re.M))
    names = {"pai_pack_max_slots", "pai_encrypt_packed", "pai_encrypt_packed_dev", "pai_decrypt_packed",
             "pai_decrypt_packed_dev"}
    assert names <= declared
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+slot_bits,\s*value_bits,\s*exponent,\s*slots;\s*\}\s*pai_pack_layout;",
                     header)
    from flex.crypto.paillier import _native
    assert names <= set(_native.EXPORTED)
    lib = _native.load_library()
    for name in names:
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is not None
    assert not [n for n in _native.EXPORTED if "FLEXPAI" in n]
    assert "PAI_OPT_OBF_CHUNK 18" in re.sub(r"\s+", " ", header) and not re.search(r"#define\s+PAI_OPT_\w+\s+19\b", header)
