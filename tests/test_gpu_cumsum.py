"""GPU parity of prefix sums of ciphertext arrays (pai_cumsum[_dev]: k_scan as row chains and as the blocked scan over
tile totals) against the reference-generated vectors (tests/golden/make_golden_cumsum.py), Context.segment_add over
explicit prefix lists, and the oracle, bit-exact; every tile length, the exponent rules, the device variant, and the
package paths down to decrypted values."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = -(1 << 31)
TAGS = [("axis0", 0, False), ("axis0_rev", 0, True), ("axis1", 1, False), ("axis1_rev", 1, True)]


def _native():
    from flex.crypto.paillier import _native as N
    return N


@pytest.fixture(scope="module")
def gcs():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_cumsum.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def key(golden):
    k = golden["keys"]["1024"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def ctx(key, xlib):
    """Public key only, on the test build."""
    return _native().Context(key.n, 0, lib=xlib)


@pytest.fixture(scope="module")
def pool(key, ctx):
    """1100 random units mod n^2 as ciphertexts with exponents 0..20 (shared, never written)."""
    N = _native()
    rng = np.random.default_rng(2048)
    M = 1100
    cs = [int.from_bytes(rng.bytes(256), "little") % key.nsquare for _ in range(M)]
    words = N.ints_to_words(cs, ctx.ct_words)
    exps = rng.integers(0, 21, M).astype(np.int32)
    words.setflags(write=False)
    exps.setflags(write=False)
    return cs, words, exps


@pytest.fixture(autouse=True)
def auto_tile(ctx):
    ctx.set_scan_tile(0)
    yield
    ctx.set_scan_tile(0)


def matches(case, tag, flat):
    if tag in case:
        return [[hex(c), e] for c, e in flat] == case[tag]
    return [hashlib.sha256(f"{hex(c)}:{e}".encode()).hexdigest() for c, e in flat] == case[tag + "_sha256"]


def draw(pool, n, seed):
    """n pool entries (with repeats): (pool indices, words, exponents)."""
    _, words, exps = pool
    idx = np.random.default_rng(seed).integers(0, exps.size, n)
    return idx, np.ascontiguousarray(words[idx]), np.ascontiguousarray(exps[idx])


def prefix_lists(outer, L, inner, rev):
    """(index, seg_off) of the prefix (suffix) of every element in array order: what a caller of pai_segment_add builds."""
    pos = np.arange(outer * L * inner, dtype=np.int64).reshape(outer, L, inner)
    lists = []
    for o in range(outer):
        for j in range(L):
            for i in range(inner):
                lists.append(pos[o, j:, i] if rev else pos[o, :j + 1, i])
    off = np.concatenate([[0], np.cumsum([m.size for m in lists])]).astype(np.int64)
    return np.concatenate(lists), off


def check_against_segment_add(ctx, words, exps, outer, L, inner, rev):
    out, oe = ctx.cumsum(words, exps, outer, L, inner, reverse=rev)
    idx, off = prefix_lists(outer, L, inner, rev)
    want, we = ctx.segment_add(words, exps, idx, off)
    assert np.array_equal(oe, we) and np.array_equal(out, want)
    return out, oe


def oracle_scan(key, cs, exps, outer, L, inner, rev):
    """[(ciphertext, exponent)] in array order: add_k over the non-empty members of every prefix, (1, EMPTY) without one."""
    res = [None] * (outer * L * inner)
    for o in range(outer):
        for i in range(inner):
            mem = []
            for j in (range(L - 1, -1, -1) if rev else range(L)):
                t = (o * L + j) * inner + i
                if exps[t] != EMPTY:
                    mem.append(t)
                res[t] = O.add_k([cs[u] for u in mem], [int(exps[u]) for u in mem], key) if mem else (1, EMPTY)
    return res


# ---------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("name", ["labels", "floats"])
def test_fixture_parity(gcs, key, ctx, name):
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.cipher_array import PaillierArray, materialize
    from flex.crypto.paillier.keypair import PaillierPublicKey
    N = _native()
    case = gcs["cases"][name]
    words = N.ints_to_words([int(h, 16) for h in case["c"]], ctx.ct_words)
    exps = np.array(case["e"], dtype=np.int32)
    enc = materialize(PaillierPublicKey(key.n), words, exps, (3, 9), obfuscated=True)
    for tag, axis, rev in TAGS:
        outer, L, inner = (1, 3, 9) if axis == 0 else (3, 9, 1)
        out, oe = ctx.cumsum(words, exps, outer, L, inner, reverse=rev)
        assert matches(case, tag, list(zip(N.words_to_ints(out), oe.tolist()))), (name, tag)
        arr = parallel_ops.cumsum(np.asarray(enc).view(np.ndarray), axis, reverse=rev)
        assert isinstance(arr, PaillierArray) and arr.shape == (3, 9)
        assert matches(case, tag, [(e.ciphertext(False), e.exponent) for e in arr.reshape(-1)]), (name, tag)


# ---------------------------------------------------------------- 2. bit-equality with the segmented add
SHAPES = [(1, 1, 1), (1, 2, 1), (5, 3, 1), (1000, 4, 1), (7, 63, 1), (7, 64, 1), (7, 65, 1), (3, 300, 2), (1, 5, 37), (2, 1025, 1)]


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_equals_segment_add(ctx, pool, shape, rev):
    outer, L, inner = shape
    _, words, exps = draw(pool, outer * L * inner, outer * 7 + L)
    assert ctx.scan_tile == 0
    check_against_segment_add(ctx, words, exps, outer, L, inner, rev)
    if shape == (1000, 4, 1):
        assert ctx.scan_path == 1
    if shape == (2, 1025, 1):
        assert ctx.scan_path == 2


# ---------------------------------------------------------------- 3. every path, the same bits
@pytest.mark.parametrize("shape", [(3, 300, 2), (1, 257, 1)])
def test_tiles_give_the_same_bits(ctx, pool, shape):
    """Tiles of 2 and 3: several scan levels of the totals; 16 and 64: ragged last tiles; 1024: one tile, the row chain."""
    outer, L, inner = shape
    _, words, exps = draw(pool, outer * L * inner, 300 + L)
    for rev in (False, True):
        want = check_against_segment_add(ctx, words, exps, outer, L, inner, rev)
        for tile in (2, 3, 16, 64, 1024):
            ctx.set_scan_tile(tile)
            assert ctx.scan_tile == tile
            got = ctx.cumsum(words, exps, outer, L, inner, reverse=rev)
            assert ctx.scan_path == (1 if tile >= L else 2)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (tile, rev)
        ctx.set_scan_tile(0)


# ---------------------------------------------------------------- 4. exponents
def exponent_rows(L, step):
    """Rows of L exponents around position `step`: the maximum rises there, an operand 20 below it there, empty entries
    leading, in the middle (at `step`), trailing, a whole row of them, and an empty run up to `step`."""
    rise = np.full(L, 3, dtype=np.int64)
    rise[step:] = 9
    low = np.full(L, 20, dtype=np.int64)
    low[step] = 0
    lead = np.full(L, 5, dtype=np.int64)
    lead[:3] = EMPTY
    mid = np.full(L, 5, dtype=np.int64)
    mid[step] = EMPTY
    mid[step + 1] = 7
    trail = np.full(L, 2, dtype=np.int64)
    trail[L - 4:] = EMPTY
    none = np.full(L, EMPTY, dtype=np.int64)
    late = np.full(L, EMPTY, dtype=np.int64)
    late[step:] = 4
    late[L - 1] = 1
    return np.stack([rise, low, lead, mid, trail, none, late])


@pytest.mark.parametrize("step", [15, 16, 17])
def test_exponent_rules(ctx, key, pool, step):
    N = _native()
    cs_pool = pool[0]
    L = 40
    E = exponent_rows(L, step)
    outer = E.shape[0]
    exps = E.reshape(-1).astype(np.int32)
    idx = np.random.default_rng(step).integers(0, len(cs_pool), exps.size)
    cs = [1 if e == EMPTY else cs_pool[t] for t, e in zip(idx.tolist(), exps.tolist())]
    words = N.ints_to_words(cs, ctx.ct_words)
    for rev in (False, True):
        want = oracle_scan(key, cs, exps.tolist(), outer, L, 1, rev)
        for tile in (0, 16):                                   # the row chain, and the step on / next to a tile boundary
            ctx.set_scan_tile(tile)
            out, oe = ctx.cumsum(words, exps, outer, L, 1, reverse=rev)
            assert list(zip(N.words_to_ints(out), oe.tolist())) == want, (rev, tile)
        ctx.set_scan_tile(0)
    # nothing has entered yet: ciphertext 1 with INT32_MIN
    out, oe = ctx.cumsum(words, exps, outer, L, 1)
    got = N.words_to_ints(out)
    assert got[2 * L] == 1 and oe[2 * L] == EMPTY and set(got[5 * L:6 * L]) == {1} and set(oe[5 * L:6 * L].tolist()) == {EMPTY}
    # the same rows as columns (inner = rows): the scan along a non-last axis
    wt = np.ascontiguousarray(words.reshape(outer, L, -1).transpose(1, 0, 2)).reshape(L * outer, -1)
    et = np.ascontiguousarray(exps.reshape(outer, L).T).reshape(-1)
    o2, e2 = ctx.cumsum(wt, et, 1, L, outer)
    assert np.array_equal(o2.reshape(L, outer, -1).transpose(1, 0, 2).reshape(out.shape), out)
    assert np.array_equal(e2.reshape(L, outer).T.reshape(-1), oe)


# ---------------------------------------------------------------- 5. uniform and mixed rows in one call
def test_uniform_and_mixed_rows_together(ctx, pool):
    outer, L = 40, 12
    _, words, exps = draw(pool, outer * L, 5)
    exps = exps.reshape(outer, L).copy()
    exps[::2] = 4                                              # every other row on one exponent
    for rev in (False, True):
        check_against_segment_add(ctx, words, exps.reshape(-1), outer, L, 1, rev)


# ---------------------------------------------------------------- 6. the device variant, argument errors
def test_dev_variant_on_a_stream(ctx, pool):
    import torch
    N = _native()
    outer, L, inner = 3, 70, 2
    _, words, exps = draw(pool, outer * L * inner, 6)
    n = exps.size
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    for tile, flags in ((0, 0), (16, N.PAI_SCAN_REVERSE)):
        ctx.set_scan_tile(tile)
        want, we = ctx.cumsum(words, exps, outer, L, inner, reverse=bool(flags))
        with torch.cuda.stream(stream):
            d_ct = torch.from_numpy(words.view(np.int32)).to(dev)
            d_ex = torch.from_numpy(exps).to(dev)
            for _ in range(2):                                 # a second call on the same context and stream
                d_out = torch.empty((n, ctx.ct_words), dtype=torch.int32, device=dev)
                d_oe = torch.empty(n, dtype=torch.int32, device=dev)
                rc = ctx.lib.pai_cumsum_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), outer, L, inner, flags,
                                            d_out.data_ptr(), d_oe.data_ptr(), stream.cuda_stream)
                assert rc == 0
                stream.synchronize()
                assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
                assert np.array_equal(d_oe.cpu().numpy(), we)
    ctx.set_scan_tile(0)
    # an overlapping output, unknown flags, a null pointer; zero sizes
    with torch.cuda.stream(stream):
        d_out = torch.empty((n, ctx.ct_words), dtype=torch.int32, device=dev)
        d_oe = torch.empty(n, dtype=torch.int32, device=dev)

        def call(ct=d_ct.data_ptr(), ex=d_ex.data_ptr(), shape=(outer, L, inner), flags=0, out=d_out.data_ptr(), oe=d_oe.data_ptr()):
            return ctx.lib.pai_cumsum_dev(ctx.handle, ct, ex, *shape, flags, out, oe, stream.cuda_stream)
        assert call() == 0
        assert call(out=d_ct.data_ptr()) == -1 and call(oe=d_ex.data_ptr()) == -1
        assert call(out=d_ct.data_ptr() + 4 * ctx.ct_words * (n - 1)) == -1          # the last row of the input
        assert call(flags=2) == -1 and call(flags=3) == -1
        assert call(ct=None) == -1 and call(ex=None) == -1 and call(out=None) == -1 and call(oe=None) == -1
        assert call(shape=(1 << 11, 1 << 10, 1 << 10)) == -1                         # 2^31 elements
        for shape in ((0, L, inner), (outer, 0, inner), (outer, L, 0)):
            assert call(shape=shape) == 0 and call(shape=shape, ct=None, ex=None, out=None, oe=None) == 0
        stream.synchronize()


def test_host_variant_argument_errors(ctx, pool):
    _, words, exps = draw(pool, 6, 9)
    out = np.empty_like(words)
    oe = np.empty_like(exps)

    def call(ct=words.ctypes.data, ex=exps.ctypes.data, shape=(1, 6, 1), flags=0, o=out.ctypes.data, e=oe.ctypes.data):
        return ctx.lib.pai_cumsum(ctx.handle, ct, ex, *shape, flags, o, e)
    assert call() == 0 and call(flags=1) == 0
    assert call(flags=4) == -1 and call(ct=None) == -1 and call(o=None) == -1 and call(o=words.ctypes.data) == -1
    assert call(shape=(0, 6, 1), ct=None, o=None) == 0 and call(shape=(1, 6, 0)) == 0
    w, e = ctx.cumsum(words[:0], exps[:0], 0, 5, 1)
    assert w.shape == (0, ctx.ct_words) and e.shape == (0,)


# ---------------------------------------------------------------- 7. key sizes
@pytest.mark.parametrize("nb", [2048, 4096])
def test_key_sizes_against_the_oracle(golden, nb):
    N = _native()
    k = golden["keys"][str(nb)]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    c = N.Context(key.n, 0)
    rng = np.random.default_rng(nb)
    cs = [int.from_bytes(rng.bytes(nb // 4), "little") % key.nsquare for _ in range(10)]
    exps = rng.integers(0, 6, 10).astype(np.int32)
    for rev in (False, True):
        out, oe = c.cumsum(N.ints_to_words(cs, c.ct_words), exps, 2, 5, 1, reverse=rev)
        assert list(zip(N.words_to_ints(out), oe.tolist())) == oracle_scan(key, cs, exps.tolist(), 2, 5, 1, rev)
    c.close()


# ---------------------------------------------------------------- 8. the package
@pytest.fixture(scope="module")
def party():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=31)
    yield pk, PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    # this key's cached context must not outlive the module (see test_gpu_fold.test_package_segment_sum_packed)
    with _runtime._lock:
        for k in [k for k in _runtime._ctxs if k[0] == pk.n]:
            _runtime._ctxs.pop(k).close()
        _runtime._private.pop(pk.n, None)


def boosting_case():
    rng = np.random.default_rng(8)
    n, F, B, nodes = 48, 3, 4, 2
    bins = rng.integers(0, B, (n, F)).astype(np.uint8)
    node = rng.integers(0, nodes, n).astype(np.int32)
    bins[(node == 1) & (bins[:, 2] == 1), 2] = 0                # cell (1, 2, 1) stays empty
    return n, F, B, nodes, bins, node, rng


def plain_hist(vals, bins, B, node, nodes):
    out = np.zeros((nodes, bins.shape[1], B) + vals.shape[1:], dtype=np.int64)
    for f in range(bins.shape[1]):
        np.add.at(out, (node, f, bins[:, f].astype(np.int64)), vals)
    return out


def test_round_trip_is_exact(party):
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, enc, dec = party
    n, F, B, nodes, bins, node, rng = boosting_case()
    y = rng.integers(-20, 21, n).astype(np.int64)
    hist, cnt = enc.encrypt_to_buffer(y).histogram(bins, B, node, nodes)
    assert cnt[1, 2, 1] == 0
    cum = hist.cumsum(axis=2)
    assert cum.shape == (nodes, F, B) and not cum.obfuscated.any()
    want = np.cumsum(plain_hist(y, bins, B, node, nodes), axis=2)
    assert np.asarray(dec.decrypt(cum)).reshape(nodes, F, B).tolist() == want.tolist()
    lay = PackedLayout.for_sum(pk, 20, 0, n)                   # sized for the cumulated sums: at most n terms of 20
    packed = cum.pack(lay, 20 * n).apply_obfuscation()
    assert packed.obfuscated
    assert np.asarray(dec.decrypt(packed)).reshape(nodes, F, B).tolist() == want.tolist()
    # suffix sums: G_R(b) including bin b
    rev = np.flip(np.cumsum(np.flip(plain_hist(y, bins, B, node, nodes), 2), 2), 2)
    assert np.asarray(dec.decrypt(hist.cumsum(2, reverse=True))).reshape(nodes, F, B).tolist() == rev.tolist()


def test_packed_histogram_cumsum(party, monkeypatch):
    from flex.crypto.paillier import _native as N
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, enc, dec = party
    n, F, B, nodes, bins, node, rng = boosting_case()
    gh = rng.integers(-1000, 1001, (n, 2)).astype(np.int64)
    lay = PackedLayout(pk, 32, 11, 0, 2)
    src = enc.encrypt_packed(gh, lay)
    src.bound = 1000
    hist, cnt = src.histogram(bins, B, node, nodes)
    out = hist.cumsum(2)
    assert out.shape == (nodes, F, B, 2) and out.bound == hist.bound * B
    want = np.cumsum(plain_hist(gh, bins, B, node, nodes), axis=2)
    assert np.asarray(dec.decrypt(out)).reshape(nodes, F, B, 2).tolist() == want.tolist()
    # the overflow refusal fires before any launch
    calls = []
    monkeypatch.setattr(N.Context, "cumsum", lambda *a, **k: calls.append(1))
    hist.bound = lay.slot_max // 2
    with pytest.raises(OverflowError):
        hist.cumsum(2)
    assert not calls


def test_sums_and_numpy_entry_points(party):
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_array import PaillierArray
    pk, enc, dec = party
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(24) * 10.0 ** rng.integers(-3, 4, 24)).reshape(2, 3, 4)
    buf = enc.encrypt_to_buffer(x)
    arr = buf.to_array()
    assert isinstance(arr, PaillierArray) and len(set(buf.exps.tolist())) > 1
    plain = np.asarray(arr).view(np.ndarray)
    pairs = lambda a: [(e.ciphertext(False), e.exponent) for e in np.asarray(a).reshape(-1)]
    calls = _runtime.context(pk).calls
    for axis in (0, 1, 2, None):
        want = plain.sum(axis=axis)                            # numpy's object reduction: the + chain on the host
        before = calls["pai_segment_add"]
        got = buf.sum(axis)
        assert list(zip(_runtime.words_to_ints(got.words), got.exps.tolist())) == pairs(want), axis
        for s in (arr.sum(axis), np.sum(arr, axis)):
            assert np.shape(s) == np.shape(want) and pairs(s) == pairs(want), axis
        assert calls["pai_segment_add"] == before + 3
        wc = np.cumsum(plain, axis)
        before = calls["pai_cumsum"]
        for s in (np.cumsum(arr, axis), arr.cumsum(axis)):
            assert isinstance(s, PaillierArray) and s.shape == wc.shape and pairs(s) == pairs(wc), axis
        assert calls["pai_cumsum"] == before + 2
        if axis is not None:
            c = buf.cumsum(axis)
            assert list(zip(_runtime.words_to_ints(c.words), c.exps.tolist())) == pairs(wc), axis
