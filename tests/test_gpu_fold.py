"""pai_pack_ciphertexts[_dev] on the GPU (csrc/kernels_pack.hpp k_pack_fold): existing ordinary ciphertexts folded into
packed ones, out_c = prod_j c_j^(16^D_j 2^(sb j)) mod n^2 with D_j = E - exp_j, and the package layer above it
(packed_buffer.pack_ciphertexts, parallel_ops.segment_sum_packed).

Expectations are Python integers:

* `fold_expected`, the definition: oracle.mul_scalar by 2^(sb j) (pow(c, 1 << (sb j), n^2), `mul_pow2`) and
  oracle.add_k, whose alignment to the largest exponent is pow(c, 16^D, n^2). One such power at the top slot of a
  4096-bit key is 4000 squarings mod n^2 on the CPU, so the cases that use it keep few contributing slots (the others
  are empty-segment entries) while the chain on the GPU keeps its full length;
* `fold_expected_c0` for the cases with many values: for unobfuscated inputs c_i = 1 + n m_i the same product is
  1 + n (sum_i m_i 16^D_i 2^(sb j) mod n), since (1 + n m)^e = 1 + n m e mod n^2 (test_fold_cpu.py checks this identity
  against the definition). These are full-width numbers mod n^2 like any other ciphertext;
* the reference's own folded ciphertexts (tests/golden/paillier_golden_fold.json);
* today's route, a chain of pai_mul by 2^sb and pai_add, which must give identical bits.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1024, 2048, 4096)
TPI = {1024: 2, 2048: 4, 4096: 8}
RK = bytes(range(33, 65))
EMPTY = -(1 << 31)


def _native():
    from flex.crypto.paillier import _native
    return _native


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


def contributes(e, E, sb):
    return e != EMPTY and 0 <= 4 * (E - e) < sb


def statuses(exps, E, sb):
    return [0 if e == EMPTY or contributes(e, E, sb) else 5 for e in exps]


def mul_pow2(c, e, bits, key):
    """c * 2^bits through oracle.mul_scalar, whose encoder takes scalars below the float range: factors of at most
    2^960 in turn (pow(pow(c, 2^a), 2^b) = pow(c, 2^(a + b)) mod n^2)."""
    c, e = O.mul_scalar(c, e, 1 << (bits % 960), key)
    for _ in range(bits // 960):
        c, e = O.mul_scalar(c, e, 1 << 960, key)
    return c, e


def fold_expected(cts, exps, lay, key):
    """The definition: per output the k-way sum, aligned to E, of c_j * 2^(sb j)."""
    sb, _, E, k = lay
    out = []
    for c0 in range(0, len(cts), k):
        terms = [mul_pow2(c, e, sb * j, key)
                 for j, (c, e) in enumerate(zip(cts[c0:c0 + k], exps[c0:c0 + k])) if contributes(e, E, sb)]
        terms.append((1, E))                      # the sum is aligned to the layout's exponent, whatever its members'
        s, e = O.add_k([t[0] for t in terms], [t[1] for t in terms], key)
        assert e == E
        out.append(s)
    return out


def fold_expected_c0(ms, exps, lay, n):
    """The same product for inputs c_i = 1 + n m_i, and the slot integers it decodes to."""
    sb, _, E, k = lay
    slots = [m << (4 * (E - e)) if contributes(e, E, sb) else 0 for m, e in zip(ms, exps)]
    cts = [(1 + n * (sum(t << (sb * j) for j, t in enumerate(slots[c:c + k])) % n)) % (n * n)
           for c in range(0, len(ms), k)]
    return cts, slots


def c0_words(ms, key, W):
    return _native().ints_to_words([(1 + key.n * (m % key.n)) % key.nsquare for m in ms], W)


@pytest.fixture(scope="module")
def golden_fold():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_fold.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def keys(golden):
    out = {}
    for nb in NBS:
        k = golden["keys"][str(nb)]
        out[nb] = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    return out


@pytest.fixture(scope="module")
def ctxs(keys):
    from test_gpu_obfuscate import _Ctxs
    made = _Ctxs(keys, None)
    yield made
    for ctx in made.cache.values():
        ctx.close()


@pytest.fixture(scope="module")
def fresh(ctxs):
    """Per key size 12 ordinary ciphertexts of small integers under the device RNG, as Python integers too: computed
    once, read by every test that needs real obfuscated inputs."""
    N = _native()
    out = {}
    for nb in NBS:
        ts = np.array([3, -5, 70000, -1, 1, 0, -(1 << 20), 12345, 7, -8, 9, -10], dtype=np.int64)
        ct, ex, st = ctxs.get(nb, "holder").encrypt(ts, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=nb)
        assert not st.any() and not ex.any()
        ct.setflags(write=False)
        out[nb] = (ts.tolist(), ct, N.words_to_ints(ct))
    return out


# ---------------------------------------------------------------- 1. the reference fixture
@pytest.mark.parametrize("party", ["holder", "public"])
@pytest.mark.parametrize("nb", NBS)
def test_reference_fixture(ctxs, keys, golden_fold, nb, party):
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, party)
    rec = golden_fold["cases"][str(nb)]
    sb, E, k = rec["slot_bits"], rec["exponent"], rec["slots"]
    lay = (sb, sb, E, k)
    exps = np.array([E - d for d in rec["delta"]], dtype=np.int32)
    assert len(rec["t"]) == 2 * k + 1 and set(rec["delta"]) == {0, 1, 2}
    words = N.ints_to_words([int(h, 16) for h in rec["ct"]], ctx.ct_words)
    out, st = ctx.pack_ciphertexts(words, exps, lay)
    assert out.shape == (3, ctx.ct_words) and not st.any()
    assert [hex(c) for c in N.words_to_ints(out)] == rec["folded"]
    want = [t << (4 * d) for t, d in zip(rec["t"], rec["delta"])]
    assert [v for h in rec["raw"] for v in unpack(int(h, 16), key.n, sb, k)][:len(want)] == want
    if party == "holder":
        val, mant, st = ctx.decrypt_packed(out, lay, len(want))
        assert not st.any() and mant.tolist() == want
        assert val.tolist() == [float(t) * 16.0 ** -E for t in want]


# ---------------------------------------------------------------- 2. the definition, at the layouts' extremes
@pytest.mark.parametrize("sb", [16, 64])
@pytest.mark.parametrize("nb", NBS)
def test_integer_product_at_the_extremes(ctxs, keys, fresh, nb, sb):
    """sb = 16 with the most slots and sb = 64: real obfuscated ciphertexts at the top slot, the bottom slot and two
    slots between, with shifts 0, 1 and the largest legal one; every other slot is an empty-segment entry, so the GPU
    walks the whole chain and the CPU computes four powers per output."""
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "public")
    ts, ct, ints = fresh[nb]
    k = (nb - 2) // sb
    E = 3
    lay = (sb, sb, E, k)
    dmax = sb // 4 - 1
    n_vals = k + 2                                           # a full output and a ragged one of two slots
    exps = np.full(n_vals, EMPTY, dtype=np.int32)
    src = np.zeros(n_vals, dtype=np.int64)
    for slot, d, which in ((k - 1, 1, 0), (k // 2, dmax, 1), (k // 2 - 1, 0, 2), (0, 0, 3), (k, dmax, 4), (k + 1, 1, 5)):
        exps[slot], src[slot] = E - d, which
    words = ct[src]
    words[exps == EMPTY] = 0
    words[exps == EMPTY, 0] = 1                              # the ciphertext 1 of an empty segment
    out, st = ctx.pack_ciphertexts(words, exps, lay)
    assert not st.any() and out.shape == (2, ctx.ct_words)
    want = fold_expected([ints[i] for i in src], exps.tolist(), lay, key)
    assert N.words_to_ints(out) == want
    # the definition once more as bare powers
    j, d = k - 1, 1
    top = pow(ints[0], 1 << (4 * d + sb * j), key.nsquare)
    rest = fold_expected([ints[i] for i in src[:k - 1]], exps[:k - 1].tolist(), lay, key)[0]
    assert want[0] == top * rest % key.nsquare


# ---------------------------------------------------------------- 3. counts, mixed exponents, signs
def _case(nb, sb, n_vals, seed):
    """(slot integers' mantissas m, exponents) of n_vals values under E = 2, one pattern per output in turn."""
    k = (nb - 2) // sb
    E, dmax = 2, sb // 4 - 1
    mx = (1 << (sb - 1)) - 1
    rng = np.random.default_rng(seed)
    ms, exps = [], []
    for i in range(n_vals):
        c, j = divmod(i, k)
        kind = c % 4
        if kind == 0:                                        # +max / -max alternating, no shift
            d, m = 0, mx if j % 2 == 0 else -mx
        elif kind == 1:                                      # all -max: the borrow runs through every slot border
            d, m = 0, -mx
        elif kind == 2:                                      # every shift in turn, the largest among them, full slots
            d = (j + c // 4) % (dmax + 1)
            m = (mx >> (4 * d)) * (1 if rng.integers(2) else -1)
        else:                                                # shifted top slot, empty-segment entries, random values
            d = dmax if j == k - 1 or i == n_vals - 1 else int(rng.integers(0, dmax + 1))
            m = int(rng.integers(-(mx >> (4 * d)), mx >> (4 * d), endpoint=True))
            if j % 5 == 2:
                d = None
        ms.append(m)
        exps.append(EMPTY if d is None else E - d)
    return ms, exps, (sb, sb, E, k)


@pytest.mark.parametrize("sb", [16, 64])
@pytest.mark.parametrize("nb", NBS)
def test_counts_mixed_exponents_and_signs(ctxs, keys, nb, sb):
    """N in {1, k - 1, k, k + 1} and (G + 1) k - 1 with G the groups of one block: a second block and a ragged last
    output. Outputs are neighbouring groups of one wave and take the patterns in turn, so the injection step differs
    inside a wave. Bits against the closed form, and the slots through pai_decrypt_packed."""
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "holder")
    k = (nb - 2) // sb
    G = 256 // TPI[nb]
    assert ctx.ct_words * 32 >= 2 * nb
    for n_vals in (1, k - 1, k, k + 1, (G + 1) * k - 1):
        ms, exps, lay = _case(nb, sb, n_vals, nb + sb + n_vals)
        want, slots = fold_expected_c0(ms, exps, lay, key.n)
        empty = [i for i, e in enumerate(exps) if e == EMPTY]
        words = c0_words([0 if e == EMPTY else m for m, e in zip(ms, exps)], key, ctx.ct_words)
        out, st = ctx.pack_ciphertexts(words, np.array(exps, dtype=np.int32), lay)
        assert out.shape == (-(-n_vals // k), ctx.ct_words) and st.shape == (n_vals,) and not st.any()
        got = N.words_to_ints(out)
        assert got == want, (n_vals, [c for c in range(len(want)) if got[c] != want[c]][:8])
        val, mant, st = ctx.decrypt_packed(out, lay, n_vals)
        assert not st.any() and mant.tolist() == slots, n_vals
        assert all(slots[i] == 0 for i in empty)
        if n_vals >= k:
            assert max(abs(t) for t in slots[:k]) == (1 << (sb - 1)) - 1


# ---------------------------------------------------------------- 4. statuses
@pytest.mark.parametrize("nb", NBS)
def test_statuses(ctxs, keys, nb):
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "holder")
    sb, E = 32, 4
    k = (nb - 2) // sb
    lay = (sb, 32, E, k)
    n_vals = 2 * k - 3
    rng = np.random.default_rng(nb)
    ms = [int(v) for v in rng.integers(-1000, 1001, n_vals)]
    exps = [E - int(d) for d in rng.integers(0, 3, n_vals)]
    bad = {0: E + 1, 3: E - 8, k - 1: E + 100, k: E - 9, k + 4: (1 << 31) - 1, n_vals - 1: -(1 << 31) + 1}
    for i, e in bad.items():
        exps[i] = e                                          # exp > E, 4 D = sb, and exponents that would wrap in 32 bits
    exps[2], exps[k + 1] = E - 7, EMPTY                      # the largest legal shift; an empty segment is not an error
    ms[2] = -5                                               # -5 * 16^7 stays inside the slot
    want, slots = fold_expected_c0(ms, exps, lay, key.n)
    out, st = ctx.pack_ciphertexts(c0_words(ms, key, ctx.ct_words), np.array(exps, dtype=np.int32), lay)
    assert st.tolist() == statuses(exps, E, sb) and sorted(np.flatnonzero(st)) == sorted(bad)
    assert set(st[list(bad)]) == {N.EL_ENC_RANGE}
    assert N.words_to_ints(out) == want
    val, mant, st2 = ctx.decrypt_packed(out, lay, n_vals)
    assert not st2.any() and mant.tolist() == slots
    assert all(mant[i] == 0 for i in bad) and mant[1] == ms[1] << (4 * (E - exps[1])) and mant[2] == ms[2] << 28
    # a null status buffer, a bad layout, null pointers
    lib = ctx.lib
    words = c0_words(ms, key, ctx.ct_words)
    ex = np.array(exps, dtype=np.int32)
    out2 = np.zeros_like(out)
    L = N.pack_layout(lay)
    assert lib.pai_pack_ciphertexts(ctx.handle, words.ctypes.data, ex.ctypes.data, n_vals, ctypes.byref(L),
                                    out2.ctypes.data, None) == 0
    assert np.array_equal(out2, out)
    for badlay in ((20, 16, 0, 3), (32, 24, 0, k + 1), (32, 24, 0, 0), (72, 64, 0, 3)):
        bl = N.pack_layout(badlay)
        assert lib.pai_pack_ciphertexts(ctx.handle, words.ctypes.data, ex.ctypes.data, n_vals, ctypes.byref(bl),
                                        out2.ctypes.data, None) == -1, badlay
    assert lib.pai_pack_ciphertexts(ctx.handle, None, ex.ctypes.data, n_vals, ctypes.byref(L), out2.ctypes.data, None) == -1
    assert lib.pai_pack_ciphertexts(ctx.handle, words.ctypes.data, ex.ctypes.data, 0, ctypes.byref(L), None, None) == 0


# ---------------------------------------------------------------- 5. parity with today's route
@pytest.mark.parametrize("nb", NBS)
def test_parity_with_the_mul_add_chain(ctxs, keys, fresh, nb):
    """k - 1 rounds of pai_mul by 2^sb and a 2-way pai_add are the only route without pai_pack_ciphertexts."""
    ctx = ctxs.get(nb, "public")
    ts, ct, ints = fresh[nb]
    sb, E, k = 32, 0, 4
    lay = (sb, 32, E, k)
    C = 3
    assert ct.shape[0] == C * k
    ex = np.zeros(C, dtype=np.int32)
    rows = ct.reshape(C, k, -1)
    acc = rows[:, k - 1].copy()
    scalar = np.array([1 << sb], dtype=np.int64)
    for j in range(k - 2, -1, -1):
        acc, e1, st = ctx.mul(acc, ex, scalar)
        assert not st.any() and not e1.any()
        acc, e2 = ctx.add([acc, rows[:, j].copy()], [ex, ex])
        assert not e2.any()
    out, st = ctx.pack_ciphertexts(ct, np.zeros(C * k, dtype=np.int32), lay)
    assert not st.any() and np.array_equal(out, acc)
    assert _native().words_to_ints(out) == fold_expected(ints, [0] * (C * k), lay, keys[nb])
    val, mant, st = ctxs.get(nb, "holder").decrypt_packed(out, lay, C * k)
    assert not st.any() and mant.tolist() == ts


# ---------------------------------------------------------------- 6. the device entry point
def test_device_entry_on_a_side_stream(ctxs, keys):
    import torch
    N = _native()
    nb, sb = 2048, 32
    key, ctx = keys[nb], ctxs.get(nb, "public")
    G = 256 // TPI[nb]
    k = (nb - 2) // sb
    n_vals = (G + 1) * k - 1
    ms, exps, lay = _case(nb, sb, n_vals, 99)
    exps[5] = lay[2] + 1                                     # one status
    words = c0_words(ms, key, ctx.ct_words)
    ex = np.array(exps, dtype=np.int32)
    out, st = ctx.pack_ciphertexts(words, ex, lay)
    assert st[5] == N.EL_ENC_RANGE and st.sum() == N.EL_ENC_RANGE
    C = out.shape[0]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_all = torch.zeros((n_vals + C, ctx.ct_words), dtype=torch.int32, device=dev)
    d_ct, d_out = d_all[:n_vals], d_all[n_vals:]
    d_ct.copy_(torch.from_numpy(words.view(np.int32)))
    d_ex = torch.from_numpy(ex).to(dev)
    d_st = torch.full((n_vals,), -1, dtype=torch.int32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    lib, L = ctx.lib, N.pack_layout(lay)
    rc = lib.pai_pack_ciphertexts_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), n_vals, ctypes.byref(L),
                                      d_out.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out)
    assert np.array_equal(d_st.cpu().numpy(), st)
    assert np.array_equal(d_ct.cpu().numpy().view(np.uint32), words), "the inputs are read only"
    # an output that overlaps the inputs: its first row on the inputs' last, and the inputs inside the output's range
    for o in (d_all[n_vals - 1:], d_all[:C], d_all[1:]):
        assert lib.pai_pack_ciphertexts_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), n_vals, ctypes.byref(L),
                                            o.data_ptr(), None, stream.cuda_stream) == -1
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out)


# ---------------------------------------------------------------- 7. the package, in an IV_FFS shape
def test_package_segment_sum_packed(monkeypatch):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=13)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    ctx = _runtime.context(pk)
    try:
        _segment_sum_packed_flow(monkeypatch, pk, enc, dec, ctx)
    finally:
        # this key's cached context must not outlive the test: while a context of the library lives, the library keeps
        # the device memory of released tables for its next build, out of reach of the test build's contexts
        with _runtime._lock:
            for key in [k for k in _runtime._ctxs if k[0] == pk.n]:
                _runtime._ctxs.pop(key).close()
            _runtime._private.pop(pk.n, None)


def _segment_sum_packed_flow(monkeypatch, pk, enc, dec, ctx):
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout, add_packed, pack_ciphertexts
    from flex.crypto.paillier.parallel_ops import segment_sum_packed
    rng = np.random.default_rng(31)
    y = rng.integers(0, 2, 300).astype(np.int64)             # the labels
    buf = enc.encrypt_to_buffer(y)
    order = rng.permutation(300)
    cuts = [0, 40, 40, 41, 120, 300]                         # bin 1 is empty, bin 2 holds one sample
    bins = [order[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    bins2 = [order[::-1][a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    sums = [int(y[b].sum()) for b in bins]
    sums2 = [int(y[b].sum()) for b in bins2]
    lay = PackedLayout.for_sum(pk, 1, 0, terms=2 * 180)      # two results of at most 180 labels each are added below
    assert lay.as_tuple() == (16, 2, 0, 63)

    def boom(*args, **kw):
        raise AssertionError("a PaillierEncryptedNumber was built on the object-free path")
    monkeypatch.setattr(PaillierEncryptedNumber, "_make", classmethod(boom))
    monkeypatch.setattr(PaillierEncryptedNumber, "__init__", boom)
    monkeypatch.setattr("flex.crypto.paillier.cipher_array._make_numbers", boom)
    pub = PaillierPublicKey(pk.n)                            # the party that sums holds the public key only
    guest = CiphertextBuffer(pub, buf.words, buf.exps)
    c0 = dict(ctx.calls)
    packed = segment_sum_packed(guest, bins, lay, 1)
    for name, cnt in (("pai_segment_add", 1), ("pai_pack_ciphertexts", 1), ("pai_add", 0), ("pai_mul", 0)):
        assert ctx.calls[name] - c0.get(name, 0) == cnt, name
    assert packed.count == 5 and packed.shape == (5,) and packed.words.shape[0] == 1
    assert packed.bound == 180 and not packed.obfuscated
    with pytest.raises(OverflowError):
        segment_sum_packed(guest, bins, PackedLayout(pub, 16, 2, 3), 1)      # 180 * 16^3 passes a 16-bit slot
    assert ctx.calls["pai_segment_add"] - c0.get("pai_segment_add", 0) == 1, "refused before any GPU call"
    before = packed.words.copy()
    wire = packed.to_wire(be_secure=True)
    assert packed.obfuscated and (packed.words != before).any()
    assert len(wire) < 5 * 4 * ctx.ct_words // 2
    back = PackedCiphertextBuffer.from_wire(wire, pk)
    got = dec.decrypt(back)
    assert got.dtype == np.int64 and got.tolist() == sums and got[1] == 0
    both = add_packed([packed, segment_sum_packed(guest, bins2, lay, 1)])
    assert both.bound == 360 and dec.decrypt(both).tolist() == [a + b for a, b in zip(sums, sums2)]
    assert dec.decrypt(both * 3).tolist() == [3 * (a + b) for a, b in zip(sums, sums2)]
    # the thin forwards: a buffer of mixed exponents, folded at the largest
    e1 = CiphertextBuffer(pub, buf.words[:70], np.where(np.arange(70) % 3 == 0, -1, 0).astype(np.int32))
    lay2 = PackedLayout(pub, 32, 32, 0)
    folded = e1.pack(lay2, 16)
    assert folded.bound == 16 and folded.count == 70 and folded.words.shape[0] == 3
    assert np.array_equal(folded.words, pack_ciphertexts(e1, lay2, 16).words)
    assert dec.decrypt(folded).tolist() == [int(v) * (16 if i % 3 == 0 else 1) for i, v in enumerate(y[:70])]
    with pytest.raises(ValueError, match="index 4"):
        CiphertextBuffer(pub, buf.words[:9], np.array([0, 0, -1, -7, -8, 0, 1, 0, 0], dtype=np.int32)).pack(lay2, 1)
    with pytest.raises(OverflowError):
        e1.pack(PackedLayout(pub, 32, 32, 8), 1)             # 16^8 = 2^32 passes the slot
