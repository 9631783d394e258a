"""pai_repack without a GPU: the Python-int fallback (packed_buffer.host_repack, PackedCiphertextBuffer.repack,
parallel_ops.repack) against the integer definition out_c = prod_j c_j^(2^(s sb j)) mod n^2 through the CPU oracle's
operators, the closed form for unobfuscated inputs that the GPU tests use, the decoded slots, the API rules, the wire, and
the refusals of the methods that address whole ciphertexts."""
import os
import re

import numpy as np
import pytest

from oracle import paillier_oracle as O
from test_fold_cpu import mul_pow2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def repack_expected(cts, stride, g, key):
    """The definition: per output the g-way sum, at one exponent, of c_j * 2^(stride j)."""
    out = []
    for c0 in range(0, len(cts), g):
        terms = [mul_pow2(c, 0, stride * j, key) for j, c in enumerate(cts[c0:c0 + g])]
        s, e = O.add_k([t[0] for t in terms], [t[1] for t in terms], key)
        assert e == 0
        out.append(s)
    return out


def repack_expected_c0(Ms, stride, g, n):
    """The same product for inputs c_i = 1 + n (M_i mod n): (1 + n m)^e = 1 + n m e mod n^2."""
    return [(1 + n * (sum(M << (stride * j) for j, M in enumerate(Ms[c:c + g])) % n)) % (n * n)
            for c in range(0, len(Ms), g)]


@pytest.fixture(scope="module")
def key1024(golden):
    k = golden["keys"]["1024"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


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


def _slots(sb, count, seed):
    """count signed slot values with the extremes +-(2^(sb - 1) - 1) among them."""
    mx = (1 << (sb - 1)) - 1
    rng = np.random.default_rng(seed)
    ts = [int(v) for v in rng.integers(-mx, mx, count, endpoint=True)]
    for i in range(count):
        if i % 3 == 0:
            ts[i] = mx if i % 2 == 0 else -mx
    return ts


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("sb,s,g", [(16, 1, 63), (24, 3, 14), (48, 2, 10), (64, 1, 15), (48, 2, 1)])
def test_host_repack_against_the_definition(key1024, sb, s, g):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_repack, pack_int
    key = key1024
    n = key.n
    pk = PaillierPublicKey(n)
    lay = PackedLayout(pk, sb, sb, 0, s)
    assert s * g <= (1024 - 2) // sb
    N = g + max(1, g - 1)                                      # a full output and one of g - 1 inputs (1 input for g <= 2)
    ts = _slots(sb, N * s, sb + s + g)
    Ms = [pack_int(ts[i * s:(i + 1) * s], sb) for i in range(N)]
    cts = [O.raw_encrypt(M % n, key, O.golden_r(n, 77, i)) for i, M in enumerate(Ms)]
    got = host_repack(cts, lay, g, pk)
    assert len(got) == -(-N // g) and all(0 < c < key.nsquare for c in got)
    assert got == repack_expected(cts, s * sb, g, key)


# ---------------------------------------------------------------- 1b. the reference fixture
@pytest.fixture(scope="module")
def golden_repack():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_repack.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("nb", [1024, 2048])
def test_reference_fixture_and_host_fallback(golden, golden_repack, nb):
    """The reference's own sum(c_j * (1 << (s sb j))) (tools/make_golden_repack.py) against host_repack, the oracle's
    operators and the decoded slots."""
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_repack, pack_int, unpack_int
    kk = golden["keys"][str(nb)]
    key = O.Key(int(kk["n"], 16), int(kk["p"], 16), int(kk["q"], 16))
    n = key.n
    pk = PaillierPublicKey(n)
    recs = golden_repack["cases"][str(nb)]
    assert [(r["slot_bits"], r["slots"]) for r in recs] == [(48, 2), (24, 3), (64, 1)]
    for case, rec in enumerate(recs):
        sb, s, g, ts = rec["slot_bits"], rec["slots"], rec["group"], rec["t"]
        cts = [int(h, 16) for h in rec["ct"]]
        assert g == (nb - 2) // sb // s and len(cts) == g + 2 and len(ts) == s * len(cts)
        mx = (1 << (sb - 1)) - 1
        assert max(ts) == mx and min(ts) == -mx
        for i in (0, g - 1, g + 1):                            # the inputs are the reference's raw_encrypt under golden_r
            M = pack_int(ts[i * s:(i + 1) * s], sb)
            assert cts[i] == O.raw_encrypt(M % n, key, O.golden_r(n, 910 + case, i)), (nb, case, i)
        got = host_repack(cts, PackedLayout(pk, sb, sb, 0, s), g, pk)
        assert [hex(c) for c in got] == rec["repacked"] and len(got) == 2
        assert got == repack_expected(cts, s * sb, g, key)
        raws = [int(h, 16) for h in rec["raw"]]
        assert [O.raw_decrypt(c, key) for c in got] == raws
        slots = [v for m in raws for v in unpack_int(m, n, sb, s * g)]
        assert slots[:len(ts)] == ts and not any(slots[len(ts):])
    assert golden_repack["gmpy2"] and golden_repack["generator"] == "tools/make_golden_repack.py"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "paillier_golden_repack.json")) < 300 * 1024


# ---------------------------------------------------------------- 2. the closed form
def test_identity_against_the_definition(key1024):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_repack, pack_int
    key = key1024
    n, nsq = key.n, key.nsquare
    pk = PaillierPublicKey(n)
    rng = np.random.default_rng(2)
    for case in range(5):
        sb = int(rng.choice([16, 24, 32, 48, 64]))
        most = (1024 - 2) // sb
        s = int(rng.integers(1, 4))
        g = int(rng.integers(2, most // s + 1))
        N = int(rng.integers(g + 1, 2 * g + 1))
        ts = _slots(sb, N * s, 100 + case)
        Ms = [pack_int(ts[i * s:(i + 1) * s], sb) for i in range(N)]
        c0 = [(1 + n * (M % n)) % nsq for M in Ms]
        want = repack_expected_c0(Ms, s * sb, g, n)
        assert want == repack_expected(c0, s * sb, g, key), (sb, s, g, N)
        assert host_repack(c0, PackedLayout(pk, sb, sb, 0, s), g, pk) == want


# ---------------------------------------------------------------- 3. the decoded slots
@pytest.mark.parametrize("sb,s,g", [(16, 1, 63), (24, 3, 14), (48, 2, 10), (64, 1, 15)])
def test_raw_plaintext_holds_the_concatenated_slots(key1024, sb, s, g):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedLayout, host_repack, pack_int, unpack_int
    key = key1024
    n = key.n
    pk = PaillierPublicKey(n)
    N = 2 * g - 1
    ts = _slots(sb, N * s, 7 * sb + g)
    cts = [O.raw_encrypt(pack_int(ts[i * s:(i + 1) * s], sb) % n, key, O.golden_r(n, 78, i)) for i in range(N)]
    got = host_repack(cts, PackedLayout(pk, sb, sb, 0, s), g, pk)
    slots = [v for c in got for v in unpack_int(O.raw_decrypt(c, key), n, sb, s * g)]
    assert slots[:len(ts)] == ts and not any(slots[len(ts):])


# ---------------------------------------------------------------- 4. the API rules
def test_api_rules(pkg):
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    from flex.crypto.paillier.parallel_ops import repack
    pk, sk, enc, dec = pkg
    lay = PackedLayout(pk, 48, 40, 2, 2)
    rng = np.random.default_rng(9)
    x = rng.integers(-1000, 1001, (2, 3, 4, 2)).astype(np.float64) / 4
    buf = enc.encrypt_packed(x, lay)
    buf.bound = 12345
    assert buf.obfuscated and buf.words.shape[0] == 24
    wide = buf.repack()
    assert isinstance(wide, PackedCiphertextBuffer)
    assert wide.layout.as_tuple() == (48, 40, 2, 20) and wide.words.shape == (3, buf.words.shape[1])
    assert wide.count == buf.count and wide.shape == buf.shape and wide.bound == 12345 and not wide.obfuscated
    got = dec.decrypt(wide)
    assert got.dtype == dec.decrypt(buf).dtype and got.shape == x.shape and np.array_equal(got, x)
    assert np.array_equal(dec.decrypt(buf), x)
    assert np.array_equal(buf.repack().words, wide.words), "deterministic: not re-randomised"
    four = repack(buf, 4)
    assert four.layout.slots == 4 and four.words.shape[0] == 12 and np.array_equal(dec.decrypt(four), x)
    assert np.array_equal(four.repack(20).words, wide.words)   # 2 -> 4 -> 20 slots are the bits of 2 -> 20
    assert buf.repack(2) is buf and repack(wide) is wide and wide.repack(20) is wide
    for bad in (3, 5, 0, -2, 1):
        with pytest.raises(ValueError, match="multiple"):
            buf.repack(bad)
    with pytest.raises(ValueError, match="do not fit"):
        buf.repack(22)                                         # (1024 - 2) // 48 = 21
    with pytest.raises(ValueError, match="multiple"):
        four.repack(6)
    with pytest.raises(TypeError):
        repack(np.arange(4))
    # operators between buffers of equal layout and shape stay valid
    both = wide + wide * 3
    assert both.bound == 4 * 12345 and np.array_equal(dec.decrypt(both), 4 * x)
    assert np.array_equal(dec.decrypt(wide - wide), 0 * x)
    with pytest.raises(ValueError, match="layouts differ"):
        wide + buf
    empty = enc.encrypt_packed(np.zeros((0, 2)), lay).repack()
    assert empty.count == 0 and empty.words.shape[0] == 0 and empty.layout.slots == 20


# ---------------------------------------------------------------- 5. the wire
def test_wire_round_trip(pkg):
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, sk, enc, dec = pkg
    lay = PackedLayout(pk, 48, 40, 0, 2)
    x = np.arange(-13, 13, dtype=np.int64).reshape(13, 2)      # 13 ciphertexts -> one full output and a ragged one
    buf = enc.encrypt_packed(x, lay)
    wide = buf.repack()
    assert wide.words.shape[0] == 2 and not wide.obfuscated
    before = wide.words.copy()
    wire = wide.to_wire(be_secure=True)
    assert wide.obfuscated and (wide.words != before).all(axis=1).any()
    assert len(buf.to_wire()) - len(wire) == 11 * 4 * buf.words.shape[1]   # 2 ciphertexts on the wire instead of 13
    back = PackedCiphertextBuffer.from_wire(wire, pk)
    assert back.layout.as_tuple() == (48, 40, 0, 20) and back.shape == (13, 2) and back.count == 26 and back.obfuscated
    got = dec.decrypt(back)
    assert got.dtype == dec.decrypt(buf).dtype and np.array_equal(got, x)
    plain = PackedCiphertextBuffer.from_wire(buf.repack().to_wire())
    assert not plain.obfuscated and np.array_equal(plain.words, before)


# ---------------------------------------------------------------- 6. whole-ciphertext methods refuse
def test_histogram_cumsum_and_take_refuse_a_repacked_buffer(pkg, monkeypatch):
    from flex.crypto.paillier import _runtime, packed_buffer
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, sk, enc, dec = pkg
    lay = PackedLayout(pk, 48, 16, 0, 2)
    cells = enc.encrypt_packed(np.ones((2, 3, 4, 2), dtype=np.int64), lay)        # a histogram's shape
    assert np.array_equal(dec.decrypt(cells.cumsum(axis=2))[0, 0, :, 0], [1, 2, 3, 4])
    assert cells.take([1], axis=0).shape == (1, 3, 4, 2)
    wide = cells.repack()
    samples = enc.encrypt_packed(np.ones((7, 2), dtype=np.int64), lay).repack()   # 7 samples: 14 values in 1 ciphertext
    whole = enc.encrypt_packed(np.ones((30, 2), dtype=np.int64), lay).repack()    # 30 samples fill 3 ciphertexts of 20
    assert whole.words.shape[0] == 3 and whole.count == 3 * whole.layout.slots

    def boom(*a, **kw):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_runtime, "context", boom)
    monkeypatch.setattr(packed_buffer, "_ints", boom)
    monkeypatch.setattr(packed_buffer, "_gpu", boom)
    with pytest.raises(ValueError, match="repack"):
        wide.cumsum(axis=2)
    with pytest.raises(ValueError, match="repack"):
        wide.take([0], axis=0)
    with pytest.raises(ValueError, match="repack"):
        samples.histogram(np.zeros((7, 1), dtype=np.uint8), 2)
    for rows in (30, 3):                                       # the samples' bins, or one row per ciphertext
        with pytest.raises(ValueError, match="repack"):
            whole.histogram(np.zeros((rows, 1), dtype=np.uint8), 2)


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_symbols():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flexpai.h")).read())
    assert ("int pai_repack(pai_ctx* ctx, const uint32_t* ct, size_t N, const pai_pack_layout* in_layout, int group, "
            "uint32_t* ct_out);") in header
    assert ("int pai_repack_dev(pai_ctx* ctx, const uint32_t* d_ct, size_t N, const pai_pack_layout* in_layout, "
            "int group, uint32_t* d_out, void* stream);") in header
    assert re.search(r"#define PAI_OPT_FOLD_ROWS 25\b", header) and re.search(r"#define PAI_OPT_FOLD_PATH 26\b", header)
    from flex.crypto.paillier import _native
    assert {"pai_repack", "pai_repack_dev"} <= set(_native.EXPORTED)
    assert (_native.PAI_OPT_FOLD_ROWS, _native.PAI_OPT_FOLD_PATH) == (25, 26)
    lib = _native.load_library()
    assert len(lib.pai_repack.argtypes) == 6 and len(lib.pai_repack_dev.argtypes) == 7
    assert callable(_native.Context.repack)
