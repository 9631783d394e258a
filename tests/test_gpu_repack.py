"""pai_repack[_dev] on the GPU, and the fold on 16-lane rows (csrc/kernels_foldw.hpp k_pack_fold_w) next to the fold on
lane groups (csrc/kernels_pack.hpp k_pack_fold) for both pai_repack and pai_pack_ciphertexts.

    out_c = prod_j ct[c g + j]^(2^(s sb j)) mod n^2

Expectations are Python integers, as in tests/test_gpu_fold.py:

* `repack_expected`, the definition: oracle.mul_scalar by 2^(stride j) (`mul_pow2`) and oracle.add_k at one exponent.
  One power at the top input of a 4096-bit key is ~4000 squarings mod n^2 on the CPU, so the cases that use it keep
  few contributing inputs (the others are the ciphertext 1) while the chain on the GPU keeps its full length;
* `repack_expected_c0`, for calls with many values: for inputs c_i = 1 + n (M_i mod n) the same product is
  1 + n (sum_j M_j 2^(stride j) mod n) (tests/test_repack_cpu.py checks this identity against the definition).

Every case runs on each path (PAI_OPT_FOLD_ROWS = 0: lane groups, 2: rows), asserts PAI_OPT_FOLD_PATH, and the two
paths must agree word for word.
"""
import ctypes

import numpy as np
import pytest

from oracle import paillier_oracle as O
from test_gpu_array_ops_sizes import K, _extremes          # noqa: F401  (K: the module fixture of the seeded keys)
from test_gpu_fold import (EMPTY, NBS, TPI, _case, c0_words, ctxs, fold_expected_c0, fresh, golden_fold,  # noqa: F401
                           keys, mul_pow2, statuses, unpack)

pytestmark = pytest.mark.gpu
PATHS = ((0, 1), (2, 2))                                   # (PAI_OPT_FOLD_ROWS, the PAI_OPT_FOLD_PATH it must give)
STRIDES = ((48, 2), (24, 3), (64, 1))                      # (sb, s): strides 96, 72 (no multiple of 28 or 32) and 64


def _native():
    from flex.crypto.paillier import _native
    return _native


def repack_expected(cts, stride, g, key):
    """The definition: per output the sum, at one exponent, of c_j * 2^(stride j); a ciphertext 1 is the factor 1."""
    out = []
    for c0 in range(0, len(cts), g):
        terms = [mul_pow2(c, 0, stride * j, key) for j, c in enumerate(cts[c0:c0 + g]) if c != 1]
        terms.append((1, 0))
        s, e = O.add_k([t[0] for t in terms], [t[1] for t in terms], key)
        assert e == 0
        out.append(s)
    return out


def repack_expected_c0(Ms, stride, g, n):
    return [(1 + n * (sum(M << (stride * j) for j, M in enumerate(Ms[c:c + g])) % n)) % (n * n)
            for c in range(0, len(Ms), g)]


def on_each_path(ctx, call):
    """call() under PAI_OPT_FOLD_ROWS = 0 and 2 (the default restored): the path is the one asked for, the outputs are
    equal; returns the output."""
    outs = []
    try:
        for mode, path in PATHS:
            ctx.set_fold_rows(mode)
            outs.append(call())
            assert ctx.fold_path == path, (mode, ctx.fold_path)
    finally:
        ctx.set_fold_rows(1)
    a, b = outs
    if isinstance(a, tuple):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "rows and lane groups differ"
    else:
        assert np.array_equal(a, b), "rows and lane groups differ"
    return a


def gmax(nb, sb, s):
    return (nb - 2) // sb // s


# ---------------------------------------------------------------- 1. the definition on real obfuscated inputs
@pytest.mark.parametrize("sb,s", STRIDES)
@pytest.mark.parametrize("nb", NBS)
def test_definition_on_obfuscated_inputs(ctxs, keys, fresh, nb, sb, s):
    """The 12 device-RNG ciphertexts as packed inputs at the top, the bottom and the middle of a chain and in a ragged
    last output; every other input is the ciphertext 1, so the GPU walks the whole chain and the CPU computes few big
    powers. g = 2 (no filler at all) and the largest g."""
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "public")
    assert ctx.fold_rows == 1 and ctx.fold_path in (0, 1, 2)
    ts, ct, ints = fresh[nb]
    W = ctx.ct_words
    lay = (sb, sb, 0, s)
    for g in (2, gmax(nb, sb, s)):
        assert g >= 2
        if g == 2:
            src = list(range(5))                              # two full outputs and one of a single input
        else:
            src = [None] * (2 * g + 2)                        # two full outputs and one of two inputs
            for pos, which in ((g - 1, 0), (g // 2, 1), (g // 2 - 1, 2), (0, 3), (2 * g - 1, 4), (g + 1, 5), (g, 6),
                               (2 * g, 7), (2 * g + 1, 8)):
                src[pos] = which
        words = np.zeros((len(src), W), dtype=np.uint32)
        words[:, 0] = 1
        for i, which in enumerate(src):
            if which is not None:
                words[i] = ct[which]
        cts = [1 if which is None else ints[which] for which in src]
        out = on_each_path(ctx, lambda: ctx.repack(words, lay, g))
        assert out.shape == (3, W)
        assert N.words_to_ints(out) == repack_expected(cts, s * sb, g, key), (nb, sb, s, g)
    # the definition once more as bare powers, at the top input of the largest g
    top = pow(ints[0], 1 << (s * sb * (g - 1)), key.nsquare)
    rest = repack_expected(cts[:g - 1], s * sb, g, key)[0]
    assert N.words_to_ints(out)[0] == top * rest % key.nsquare
    # the plaintext is the one pai_decrypt_packed decodes under (sb, vb, e, s g): slot 0 of each input holds its integer
    val, mant, st = ctxs.get(nb, "holder").decrypt_packed(out, (sb, sb, 0, s * g), len(src) * s)
    assert not st.any()
    assert mant.tolist() == [v for which in src for v in ([0 if which is None else ts[which]] + [0] * (s - 1))]


# ---------------------------------------------------------------- 1b. the reference fixture
@pytest.fixture(scope="module")
def golden_repack():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "paillier_golden_repack.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("party", ["holder", "public"])
@pytest.mark.parametrize("nb", [1024, 2048])
def test_reference_fixture(ctxs, keys, golden_repack, nb, party):
    """The reference's own sum(c_j * (1 << (s sb j))) through PaillierEncryptedNumber.__mul__ and __add__
    (tools/make_golden_repack.py), on each path."""
    N = _native()
    ctx = ctxs.get(nb, party)
    for rec in golden_repack["cases"][str(nb)]:
        sb, s, g = rec["slot_bits"], rec["slots"], rec["group"]
        words = N.ints_to_words([int(h, 16) for h in rec["ct"]], ctx.ct_words)
        out = on_each_path(ctx, lambda: ctx.repack(words, (sb, sb, 0, s), g))
        assert [hex(c) for c in N.words_to_ints(out)] == rec["repacked"], (nb, sb, s)
        if party == "holder":
            val, mant, st = ctx.decrypt_packed(out, (sb, sb, 0, s * g), len(rec["t"]))
            assert not st.any() and mant.tolist() == rec["t"]


# ---------------------------------------------------------------- 2. seams
@pytest.mark.parametrize("nb", NBS)
def test_seams(ctxs, keys, nb):
    """Output counts around the four rows of a wave, around the group kernel's block, and 4 097; a last output of one
    input and one of g - 1 inputs, so that the rows (groups) of one wave start at different top slots. Inputs
    c = 1 + n M with both slots at random signed values and at +-bound; bits against the closed form."""
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "holder")
    n = key.n
    sb, s, g = 48, 2, 4
    lay = (sb, sb, 0, s)
    G = 256 // TPI[nb]
    mx = (1 << (sb - 1)) - 1
    rng = np.random.default_rng(nb)
    most = 4097 * g
    ts = rng.integers(-mx, mx, (most, s), endpoint=True)
    ts[::7] = mx
    ts[3::7] = -mx
    Ms = [int(a) + (int(b) << sb) for a, b in ts.tolist()]
    words = c0_words(Ms, key, ctx.ct_words)
    for C in (1, 3, 4, 5, G - 1, G + 1, 4097):
        for last in (1, g - 1):
            n_in = (C - 1) * g + last
            out = on_each_path(ctx, lambda: ctx.repack(words[:n_in], lay, g))
            assert out.shape == (C, ctx.ct_words)
            got, want = N.words_to_ints(out), repack_expected_c0(Ms[:n_in], s * sb, g, n)
            assert got == want, (C, last, [c for c in range(C) if got[c] != want[c]][:8])
    n_in = 4 * g + 1
    val, mant, st = ctx.decrypt_packed(ctx.repack(words[:n_in], lay, g), (sb, sb, 0, s * g), n_in * s)
    assert not st.any() and mant.tolist() == ts[:n_in].reshape(-1).tolist()


# ---------------------------------------------------------------- 3. edge residues at the ends of a chain
@pytest.mark.parametrize("name", ["K1035T", "K2071T", "K3072"])
def test_edge_residues_at_the_ends_of_a_chain(K, name):
    """n^2 - 1, n^2 - 2, n + 1, (n^2 -+ 1) / 2 and 1 as the top and the bottom input of a chain of the largest g (the
    inputs between are the ciphertext 1), at the keys where 4 n^2 sits next to the group engine's R = 2^(28 * 37 * TPI),
    which is the rows' R too, and at 3072 bits."""
    N = _native()
    ctx, key = K.public(name)
    nb = key.n.bit_length()
    sb, s = 48, 2
    g = gmax(nb, sb, s)
    x = _extremes(key)
    cts = []
    for i in range(len(x)):                                    # output i: bottom x[i], top x[(i + 2) % 6]
        cts += [x[i]] + [1] * (g - 2) + [x[(i + 2) % len(x)]]
    cts += [x[0], x[5]]                                        # a ragged output: both ends next to each other
    words = N.ints_to_words(cts, ctx.ct_words)
    out = on_each_path(ctx, lambda: ctx.repack(words, (sb, sb, 0, s), g))
    assert out.shape == (len(x) + 1, ctx.ct_words)
    want = repack_expected(cts, s * sb, g, key)
    assert N.words_to_ints(out) == want
    assert want[3] == pow(x[5], 1 << (s * sb * (g - 1)), key.nsquare)          # bottom 1, top n^2 - 2


# ---------------------------------------------------------------- 4. pai_pack_ciphertexts on rows
@pytest.mark.parametrize("party", ["holder", "public"])
@pytest.mark.parametrize("nb", NBS)
def test_pack_ciphertexts_reference_fixture_on_each_path(ctxs, keys, golden_fold, nb, party):
    N = _native()
    ctx = ctxs.get(nb, party)
    rec = golden_fold["cases"][str(nb)]
    sb, E, k = rec["slot_bits"], rec["exponent"], rec["slots"]
    exps = np.array([E - d for d in rec["delta"]], dtype=np.int32)
    words = N.ints_to_words([int(h, 16) for h in rec["ct"]], ctx.ct_words)
    out, st = on_each_path(ctx, lambda: ctx.pack_ciphertexts(words, exps, (sb, sb, E, k)))
    assert not st.any() and [hex(c) for c in N.words_to_ints(out)] == rec["folded"]


@pytest.mark.parametrize("sb", [16, 64])
@pytest.mark.parametrize("nb", NBS)
def test_pack_ciphertexts_mixed_exponents_on_each_path(ctxs, keys, nb, sb):
    """test_gpu_fold's patterns (every shift in turn, empty-segment entries, +-max) over five outputs, the last ragged:
    the injection step differs between the rows of a wave."""
    N = _native()
    key, ctx = keys[nb], ctxs.get(nb, "holder")
    k = (nb - 2) // sb
    n_vals = 5 * k - 3
    ms, exps, lay = _case(nb, sb, n_vals, nb + sb)
    want, slots = fold_expected_c0(ms, exps, lay, key.n)
    words = c0_words([0 if e == EMPTY else m for m, e in zip(ms, exps)], key, ctx.ct_words)
    out, st = on_each_path(ctx, lambda: ctx.pack_ciphertexts(words, np.array(exps, dtype=np.int32), lay))
    assert not st.any() and N.words_to_ints(out) == want
    val, mant, st = ctx.decrypt_packed(out, lay, n_vals)
    assert not st.any() and mant.tolist() == slots


@pytest.mark.parametrize("nb", NBS)
def test_pack_ciphertexts_statuses_on_each_path(ctxs, keys, nb):
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
        exps[i] = e
    exps[2], exps[k + 1] = E - 7, EMPTY
    ms[2] = -5
    want, slots = fold_expected_c0(ms, exps, lay, key.n)
    words = c0_words(ms, key, ctx.ct_words)
    out, st = on_each_path(ctx, lambda: ctx.pack_ciphertexts(words, np.array(exps, dtype=np.int32), lay))
    assert st.tolist() == statuses(exps, E, sb) and sorted(np.flatnonzero(st)) == sorted(bad)
    assert N.words_to_ints(out) == want


# ---------------------------------------------------------------- 5. arguments
def test_arguments(ctxs, keys):
    N = _native()
    nb = 1024
    key, ctx = keys[nb], ctxs.get(nb, "holder")
    lib, h, W = ctx.lib, ctx.handle, ctx.ct_words
    sb, s, g = 48, 2, 10
    words = c0_words(list(range(1, 26)), key, W)
    out = np.zeros((3, W), dtype=np.uint32)
    L = N.pack_layout((sb, sb, 0, s))
    ok = lambda *a: lib.pai_repack(h, *a)
    assert ok(words.ctypes.data, 25, ctypes.byref(L), g, out.ctypes.data) == 0
    assert N.words_to_ints(out) == repack_expected_c0(list(range(1, 26)), s * sb, g, key.n)
    before = out.copy()
    assert ok(None, 25, ctypes.byref(L), g, out.ctypes.data) == -1
    assert ok(words.ctypes.data, 25, ctypes.byref(L), g, None) == -1
    assert ok(words.ctypes.data, 25, None, g, out.ctypes.data) == -1
    for bad_g in (0, -1, 11, 1 << 30):                         # s g = 22 > (1024 - 2) // 48 = 21
        assert ok(words.ctypes.data, 25, ctypes.byref(L), bad_g, out.ctypes.data) == -1, bad_g
    for badlay in ((20, 16, 0, 2), (48, 49, 0, 2), (48, 1, 0, 2), (48, 48, 0, 0), (48, 48, 0, 22), (72, 64, 0, 2),
                   (96, 48, 0, 1)):
        bl = N.pack_layout(badlay)
        assert ok(words.ctypes.data, 25, ctypes.byref(bl), 1, out.ctypes.data) == -1, badlay
    # an output that overlaps the input: on the inputs' first and last rows
    assert ok(words.ctypes.data, 25, ctypes.byref(L), g, words.ctypes.data) == -1
    assert ok(words.ctypes.data, 25, ctypes.byref(L), g, words[24:].ctypes.data) == -1
    assert ok(words[2:].ctypes.data, 23, ctypes.byref(L), g, words.ctypes.data) == -1
    assert np.array_equal(out, before) and np.array_equal(words, c0_words(list(range(1, 26)), key, W))
    # N = 0 is PAI_OK, whatever the buffers; group 1 copies
    assert ok(None, 0, ctypes.byref(L), g, None) == 0
    assert np.array_equal(ctx.repack(words, (sb, sb, 0, s), 1), words)
    assert ctx.repack(words[:0], (sb, sb, 0, s), g).shape == (0, W)
    # the options
    assert lib.pai_ctx_set_option(h, N.PAI_OPT_FOLD_ROWS, 3) == -1 and lib.pai_ctx_set_option(h, N.PAI_OPT_FOLD_ROWS, -1) == -1
    assert lib.pai_ctx_set_option(h, N.PAI_OPT_FOLD_PATH, 1) == -1 and ctx.fold_rows == 1
    # a slot of the three older entry points stays at most 64 bits wide
    ex = np.zeros(25, dtype=np.int32)
    st = np.zeros(25, dtype=np.int32)
    x = np.zeros(25, dtype=np.int64)
    val = np.zeros(25, dtype=np.float64)
    for badlay in ((72, 64, 0, 2), (96, 48, 0, 2), (96, 96, 0, 1)):
        bl = N.pack_layout(badlay)
        assert lib.pai_pack_ciphertexts(h, words.ctypes.data, ex.ctypes.data, 25, ctypes.byref(bl), out.ctypes.data,
                                        st.ctypes.data) == -1, badlay
        assert lib.pai_encrypt_packed(h, N.PAI_I64, x.ctypes.data, 2, ctypes.byref(bl), N.PAI_OBF_NONE, None, 0, 0, None, 0,
                                      out.ctypes.data, st.ctypes.data) == -1, badlay
        assert lib.pai_decrypt_packed(h, words.ctypes.data, ctypes.byref(bl), 2, val.ctypes.data, None,
                                      st.ctypes.data) == -1, badlay
        got = ctypes.c_int(-7)
        assert lib.pai_pack_max_slots(h, badlay[0], ctypes.byref(got)) == -1 and got.value == -7


# ---------------------------------------------------------------- 6. the device entry point
def test_device_entry_on_a_side_stream(ctxs, keys):
    import torch
    N = _native()
    nb, sb, s, g = 2048, 48, 2, 21
    key, ctx = keys[nb], ctxs.get(nb, "public")
    G = 256 // TPI[nb]
    n_in = (G + 1) * g - 1
    rng = np.random.default_rng(5)
    Ms = [int(v) for v in rng.integers(-(1 << 62), 1 << 62, n_in)]
    words = c0_words(Ms, key, ctx.ct_words)
    lay = (sb, sb, 0, s)
    want = on_each_path(ctx, lambda: ctx.repack(words, lay, g))
    C = want.shape[0]
    assert C == G + 1 and N.words_to_ints(want) == repack_expected_c0(Ms, s * sb, g, key.n)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_all = torch.zeros((n_in + C, ctx.ct_words), dtype=torch.int32, device=dev)
    d_ct, d_out = d_all[:n_in], d_all[n_in:]
    d_ct.copy_(torch.from_numpy(words.view(np.int32)))
    stream.wait_stream(torch.cuda.current_stream(dev))
    lib, L = ctx.lib, N.pack_layout(lay)
    try:
        for mode, path in PATHS:
            ctx.set_fold_rows(mode)
            d_out.zero_()
            stream.wait_stream(torch.cuda.current_stream(dev))
            rc = lib.pai_repack_dev(ctx.handle, d_ct.data_ptr(), n_in, ctypes.byref(L), g, d_out.data_ptr(),
                                    stream.cuda_stream)
            assert rc == 0, lib.pai_last_error().decode()
            stream.synchronize()
            assert ctx.fold_path == path
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
            assert np.array_equal(d_ct.cpu().numpy().view(np.uint32), words), "the inputs are read only"
    finally:
        ctx.set_fold_rows(1)
    # an output that overlaps the inputs: its first row on the inputs' last, and the inputs inside the output's range
    for o in (d_all[n_in - 1:], d_all[:C], d_all[1:]):
        assert lib.pai_repack_dev(ctx.handle, d_ct.data_ptr(), n_in, ctypes.byref(L), g, o.data_ptr(),
                                  stream.cuda_stream) == -1
    assert lib.pai_repack_dev(ctx.handle, None, n_in, ctypes.byref(L), g, d_out.data_ptr(), stream.cuda_stream) == -1
    assert lib.pai_repack_dev(ctx.handle, d_ct.data_ptr(), n_in, ctypes.byref(L), 22, d_out.data_ptr(),
                              stream.cuda_stream) == -1
    assert lib.pai_repack_dev(ctx.handle, None, 0, ctypes.byref(L), g, None, stream.cuda_stream) == 0
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


# ---------------------------------------------------------------- 7. the package, one boosting level
@pytest.fixture(scope="module")
def party():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=17)
    yield pk, PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    # this key's cached context must not outlive the module (see test_gpu_fold.test_package_segment_sum_packed)
    with _runtime._lock:
        for k in [k for k in _runtime._ctxs if k[0] == pk.n]:
            _runtime._ctxs.pop(k).close()
        _runtime._private.pop(pk.n, None)


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_package_flow(party, resident):
    from flex.crypto.paillier import _runtime, parallel_ops
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, enc, dec = party
    rng = np.random.default_rng(12)
    n, F, B, nodes = 300, 3, 4, 2
    bins = rng.integers(0, B, (n, F)).astype(np.uint8)
    node = rng.integers(0, nodes, n).astype(np.int32)
    bins[(node == 1) & (bins[:, 2] == 1), 2] = 0               # cell (1, 2, 1) stays empty
    gh = rng.integers(-4096, 4097, (n, 2)).astype(np.float64) / 4096           # exact at exponent 3
    lay = PackedLayout(pk, 48, 14, 3, 2)
    src = enc.encrypt_packed(gh, lay)
    if resident:
        src = src.to_device()
    hist, cnt = src.histogram(bins, B, node, nodes)
    assert cnt[1, 2, 1] == 0
    left = hist.cumsum(axis=2)
    assert left.shape == (nodes, F, B, 2) and left.words.shape[0] == 24 and left.resident == resident
    calls = _runtime.context(pk).calls
    name = "pai_repack_dev" if resident else "pai_repack"
    before = calls[name]
    wide = left.repack()
    assert calls[name] == before + 1
    g = (1024 - 2) // 48 // 2
    assert wide.layout.as_tuple() == (48, 14, 3, 2 * g) and wide.words.shape[0] == -(-24 // g) == 3
    assert wide.resident == resident and not wide.obfuscated
    assert wide.shape == left.shape and wide.count == left.count and wide.bound == left.bound
    assert parallel_ops.repack(left).layout == wide.layout
    wire = wide.to_wire(be_secure=True)
    plain_wire = left.to_wire(be_secure=True)
    W = wide.words.shape[1]
    assert len(plain_wire) - len(wire) == (24 - 3) * 4 * W
    want = np.cumsum(_plain_hist(gh, bins, B, node, nodes), axis=2)
    for w, C in ((wire, 3), (plain_wire, 24)):
        back = PackedCiphertextBuffer.from_wire(w, PaillierPublicKey(pk.n), device=resident)
        assert back.words.shape[0] == C and back.obfuscated and back.resident == resident
        got = dec.decrypt(back)
        assert got.dtype == np.float64 and got.shape == (nodes, F, B, 2)
        assert np.array_equal(got, want)
    assert (want[1, 2, 1] == want[1, 2, 0]).all()
    with pytest.raises(ValueError, match="repack"):
        wide.cumsum(axis=2)
    with pytest.raises(ValueError, match="repack"):
        wide.take([0], axis=0)


def _plain_hist(vals, bins, B, node, nodes):
    out = np.zeros((nodes, bins.shape[1], B) + vals.shape[1:], dtype=np.float64)
    for f in range(bins.shape[1]):
        np.add.at(out, (node, f, bins[:, f].astype(np.int64)), vals)
    return out
