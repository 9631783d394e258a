"""GPU parity of encrypted histograms (pai_histogram[_dev]: k_hist_count, k_hist_scatter, k_hist_acc over the runs or,
on the test build, k_hist_rows + k_add, the segmented add over the runs' partials) against the reference-generated vectors
(tests/golden/make_golden_hist.py), Context.segment_add over lists built from the same bins, and the oracle, bit-exact;
the feature blocks, the host variant's chunks, the device variant, and the package paths down to decrypted values."""
import json
import math
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = -(1 << 31)


def _native():
    from flex.crypto.paillier import _native as N
    return N


@pytest.fixture(scope="module")
def ghist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_hist.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def key(golden):
    k = golden["keys"]["1024"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def ctx(key, xlib):
    """Public key only, on the test build (it reads the scratch budget and the chunk size from the environment)."""
    return _native().Context(key.n, 0, lib=xlib)


@pytest.fixture(scope="module")
def pool(key, ctx):
    """1100 random units mod n^2 as ciphertexts with exponents 0..20 (shared, never written)."""
    N = _native()
    rng = np.random.default_rng(1024)
    M = 16 * N.HIST_RUN + 1 + 70
    cs = [int.from_bytes(rng.bytes(256), "little") % key.nsquare for _ in range(M)]
    words = N.ints_to_words(cs, ctx.ct_words)
    exps = rng.integers(0, 21, M).astype(np.int32)
    words.setflags(write=False)
    exps.setflags(write=False)
    return cs, words, exps


def lists_from_bins(bins, B, node, nodes):
    """(index, seg_off) of the cells (v, f, b) in order: what a caller of pai_segment_add builds."""
    n, F = bins.shape
    v = np.zeros(n, dtype=np.int64) if node is None else np.asarray(node, dtype=np.int64)
    members = []
    for vv in range(nodes):
        for f in range(F):
            for b in range(B):
                members.append(np.flatnonzero((v == vv) & (bins[:, f] == b)))
    idx = np.concatenate(members).astype(np.int64) if members else np.zeros(0, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum([m.size for m in members])]).astype(np.int64)
    return idx, off


def check_against_segment_add(ctx, words, exps, bins, B, node, nodes):
    out, oe, cnt = ctx.histogram(words, exps, bins, B, node, nodes)
    idx, off = lists_from_bins(bins, B, node, nodes)
    want, we = ctx.segment_add(words, exps, idx, off)
    assert np.array_equal(cnt, np.diff(off))
    assert np.array_equal(oe, we) and np.array_equal(out, want)
    assert np.all(oe[cnt == 0] == EMPTY)
    return out, oe, cnt


# ---------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("name", ["labels", "floats"])
def test_fixture_parity(ghist, key, ctx, name):
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.cipher_array import materialize
    from flex.crypto.paillier.keypair import PaillierPublicKey
    N = _native()
    case = ghist["cases"][name]
    F, B, nodes = ghist["F"], ghist["B"], ghist["nodes"]
    words = N.ints_to_words([int(h, 16) for h in case["c"]], ctx.ct_words)
    exps = np.array(case["e"], dtype=np.int32)
    bins = np.array(ghist["bins"], dtype=np.uint8)
    node = np.array(ghist["node"], dtype=np.int32)
    out, oe, cnt = ctx.histogram(words, exps, bins, B, node, nodes)
    assert cnt.tolist() == case["counts"] and cnt.dtype == np.int64
    got = N.words_to_ints(out)
    for s, cell in enumerate(case["cells"]):
        if cell is None:
            assert got[s] == 1 and int(oe[s]) == EMPTY
        else:
            assert [hex(got[s]), int(oe[s])] == cell, (name, s)
    pub = PaillierPublicKey(key.n)
    arr, c2 = parallel_ops.histogram(materialize(pub, words, exps, (48,), obfuscated=True), bins, B, node, nodes)
    assert arr.shape == (nodes, F, B) and c2.reshape(-1).tolist() == case["counts"]
    for s, e in enumerate(np.asarray(arr).reshape(-1)):
        want = [hex(1), 0] if case["cells"][s] is None else case["cells"][s]
        assert [hex(e.ciphertext(False)), e.exponent] == want, (name, s)


# ---------------------------------------------------------------- 2. bit-equality with the segmented add
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("F,B,dtype,nodes", [(1, 1, np.uint8, 1), (3, 2, np.uint8, 5), (17, 256, np.uint8, 1),
                                             (3, 300, np.uint16, 5), (17, 2, np.uint16, 1)])
def test_equals_segment_add(ctx, pool, n, F, B, dtype, nodes):
    _, words, exps = pool
    rng = np.random.default_rng(n * 1000 + F * 10 + nodes)
    hi = min(B, 7) + 1                                         # a few populated bins, the last id out of range
    wide = rng.integers(0, hi, (n, F + 3)).astype(dtype)
    if B <= np.iinfo(dtype).max:
        wide[wide == hi - 1] = B                               # missing (uint8 has no id beyond 256 bins)
    if B > 2:
        wide[0, 0] = B - 1                                     # the last bin is reachable
    bins = wide[:, :F]                                         # bin_stride > F
    node = None if nodes == 1 else rng.integers(-1, nodes + 1, n).astype(np.int32)
    check_against_segment_add(ctx, words[:n], exps[:n], bins, B, node, nodes)


def test_one_cell_holds_every_sample(ctx, pool):
    """HIST_RUN, HIST_RUN +- 1 members in one run or two, and 16 HIST_RUN + 1: 17 runs, a second level of the closing
    tree."""
    R = _native().HIST_RUN
    _, words, exps = pool
    for n in (R - 1, R, R + 1, 16 * R + 1):
        bins = np.full((n, 2), 3, dtype=np.uint8)
        bins[:, 1] = 9                                         # feature 1: every sample missing
        out, oe, cnt = check_against_segment_add(ctx, words[:n], exps[:n], bins, 5, None, 1)
        assert cnt.tolist() == [0, 0, 0, n, 0] + [0] * 5


def test_argument_errors(ctx, pool):
    N = _native()
    _, words, exps = pool
    w, e = np.ascontiguousarray(words[:4]), np.ascontiguousarray(exps[:4])
    bins = np.zeros((4, 2), dtype=np.uint8)
    out = np.empty((8, ctx.ct_words), dtype=np.uint32)
    oe = np.empty(8, dtype=np.int32)
    node = np.zeros(4, dtype=np.int32)

    def call(F=2, stride=2, nd=None, nodes=1, B=2, dt=N.PAI_BIN_U8, n=4, o=out.ctypes.data):
        return ctx.lib.pai_histogram(ctx.handle, w.ctypes.data, e.ctypes.data, n, dt, bins.ctypes.data, F, stride,
                                     nd, nodes, B, o, oe.ctypes.data, None)
    assert call() == 0
    assert call(stride=1) == -1 and call(B=0) == -1 and call(B=257) == -1 and call(nodes=0) == -1 and call(nodes=2) == -1
    assert call(dt=2) == -1 and call(o=None) == -1 and call(F=0, stride=0) == -1
    assert call(dt=N.PAI_BIN_U16, B=65537, F=1) == -1
    assert call(nd=node.ctypes.data, nodes=1 << 23, B=2) == -1            # 2^25 cells
    assert call(n=1 << 30) == -1                                          # N F = 2^31


# ---------------------------------------------------------------- 3. key sizes
@pytest.mark.parametrize("nb", [1024, 2048, 4096])
def test_key_sizes_against_the_oracle(golden, nb):
    N = _native()
    k = golden["keys"][str(nb)]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    c = N.Context(key.n, 0)
    n, F, B = 200, 2, 3
    rng = np.random.default_rng(nb)
    cs = [int.from_bytes(rng.bytes(nb // 4), "little") % key.nsquare for _ in range(n)]
    exps = rng.integers(0, 21, n).astype(np.int32)
    bins = rng.integers(0, B + 1, (n, F)).astype(np.uint8)
    out, oe, cnt = c.histogram(N.ints_to_words(cs, c.ct_words), exps, bins, B)
    got = N.words_to_ints(out)
    for f in range(F):
        for b in range(B):
            mem = np.flatnonzero(bins[:, f] == b).tolist()
            assert mem and cnt[f * B + b] == len(mem)
            assert (got[f * B + b], int(oe[f * B + b])) == O.add_k([cs[i] for i in mem], [int(exps[i]) for i in mem], key)


# ---------------------------------------------------------------- 4. feature blocks, host chunks, variants
VARIANTS = [{"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "64"}, {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "7"},
            {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "256"}, {"FLEXPAI_HIST_ACC": "0"}]
HIST_ENV = ("FLEXPAI_HIST_ACC", "FLEXPAI_HIST_RUN", "FLEXPAI_HIST_SCRATCH_BYTES", "FLEXPAI_HIST_CHUNK")


def _set(monkeypatch, env):
    for k in HIST_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                               # read by the test build only, at every call


def test_blocks_and_chunks_give_the_same_bits(ctx, pool, monkeypatch):
    _, words, exps = pool
    n, F, B, nodes = 300, 17, 4, 2
    rng = np.random.default_rng(17)
    bins = rng.integers(0, B + 1, (n, F)).astype(np.uint8)
    node = rng.integers(-1, nodes + 1, n).astype(np.int32)
    _set(monkeypatch, {})
    want = ctx.histogram(words[:n], exps[:n], bins, B, node, nodes)
    assert want[2].reshape(nodes, F, B).sum(axis=(0, 2)).min() >= 80     # members per feature: 320 bytes of list and more
    for var in VARIANTS:
        # 1500 bytes: four features' member lists at the most (one feature with the 512-byte gather rows of k_add), so
        # 17 features take five blocks or more; 1 byte: a block per feature, and five chunks of samples, the last ragged
        for extra in ({"FLEXPAI_HIST_SCRATCH_BYTES": "1500"}, {"FLEXPAI_HIST_SCRATCH_BYTES": "1", "FLEXPAI_HIST_CHUNK": "70"}):
            _set(monkeypatch, dict(var, **extra))
            got = ctx.histogram(words[:n], exps[:n], bins, B, node, nodes)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (var, extra)


def test_run_lengths_and_variants(ctx, pool, monkeypatch):
    """One cell of 16 HIST_RUN + 1 members on two exponent levels of more than 64 members per run: k_hist_acc restores
    the Montgomery factor inside a level. Every variant and run length gives the bits of the segmented add."""
    R = _native().HIST_RUN
    _, words, _ = pool
    n = 16 * R + 1
    exps = np.where(np.arange(n) % 3 == 0, 2, 5).astype(np.int32)
    bins = np.zeros((n, 1), dtype=np.uint8)
    for var in VARIANTS + [{"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "128"}, {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "2000"}]:
        _set(monkeypatch, var)
        check_against_segment_add(ctx, words[:n], exps, bins, 2, None, 1)


# ---------------------------------------------------------------- 5. the device variant
def test_dev_variant_on_a_stream(ctx, pool):
    import torch
    N = _native()
    _, words, exps = pool
    n, F, B, nodes = 500, 5, 6, 3
    rng = np.random.default_rng(5)
    wide = rng.integers(0, B + 1, (n, F + 2)).astype(np.uint16)
    node = rng.integers(-1, nodes + 1, n).astype(np.int32)
    want, we, wc = ctx.histogram(words[:n], exps[:n], wide[:, :F], B, node, nodes)
    cells = nodes * F * B
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_ct = torch.from_numpy(words[:n].copy().view(np.int32)).to(dev)
        d_ex = torch.from_numpy(exps[:n].copy()).to(dev)
        d_bins = torch.from_numpy(wide.view(np.int16)).to(dev)
        d_node = torch.from_numpy(node).to(dev)
        for _ in range(2):                                     # a second call on the same context and stream
            d_out = torch.empty((cells, ctx.ct_words), dtype=torch.int32, device=dev)
            d_oe = torch.empty(cells, dtype=torch.int32, device=dev)
            d_cnt = torch.empty(cells, dtype=torch.int64, device=dev)
            rc = ctx.lib.pai_histogram_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), n, N.PAI_BIN_U16, d_bins.data_ptr(),
                                           F, F + 2, d_node.data_ptr(), nodes, B, d_out.data_ptr(), d_oe.data_ptr(),
                                           d_cnt.data_ptr(), stream.cuda_stream)
            assert rc == 0
            stream.synchronize()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
            assert np.array_equal(d_oe.cpu().numpy(), we) and np.array_equal(d_cnt.cpu().numpy(), wc)
        # without counts
        d_out = torch.empty((cells, ctx.ct_words), dtype=torch.int32, device=dev)
        rc = ctx.lib.pai_histogram_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), n, N.PAI_BIN_U16, d_bins.data_ptr(), F,
                                       F + 2, d_node.data_ptr(), nodes, B, d_out.data_ptr(), d_oe.data_ptr(), None,
                                       stream.cuda_stream)
        assert rc == 0
        stream.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


# ---------------------------------------------------------------- 6, 7. the package
@pytest.fixture(scope="module")
def party():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=29)
    yield pk, PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    # this key's cached context must not outlive the module (see test_gpu_fold.test_package_segment_sum_packed)
    with _runtime._lock:
        for k in [k for k in _runtime._ctxs if k[0] == pk.n]:
            _runtime._ctxs.pop(k).close()
        _runtime._private.pop(pk.n, None)


def test_round_trip_is_exact(party):
    pk, enc, dec = party
    rng = np.random.default_rng(6)
    n, F, B, nodes = 400, 3, 5, 2
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    bins = rng.integers(0, B + 1, (n, F)).astype(np.uint8)
    bins[:, 2] = np.minimum(bins[:, 2], B - 2) if B > 1 else 0          # (feature 2, bin 4) empty
    node = rng.integers(-1, nodes + 1, n).astype(np.int32)
    buf = enc.encrypt_to_buffer(x)
    decoded = dec.decrypt(buf)                                          # the members' decoded values
    out, cnt = buf.histogram(bins, B, node, nodes)
    assert out.shape == cnt.shape == (nodes, F, B) and not out.obfuscated.any()
    got = np.asarray(dec.decrypt(out)).reshape(nodes, F, B)
    for v in range(nodes):
        for f in range(F):
            for b in range(B):
                mem = np.flatnonzero((node == v) & (bins[:, f] == b))
                assert cnt[v, f, b] == mem.size
                assert got[v, f, b] == math.fsum(decoded[mem].tolist()), (v, f, b)
    assert cnt[0, 2, B - 1] == 0 and got[0, 2, B - 1] == 0 and (out.exps[cnt.reshape(-1) == 0] == 0).all()


def test_packed_paths(party, monkeypatch):
    from flex.crypto.paillier import _native as N
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, enc, dec = party
    rng = np.random.default_rng(7)
    n, F, B, nodes = 300, 4, 3, 2
    y = rng.integers(0, 2, n).astype(np.int64)
    bins = rng.integers(0, B + 1, (n, F)).astype(np.uint8)
    node = rng.integers(0, nodes, n).astype(np.int32)
    ones = np.zeros((nodes, F, B), dtype=np.int64)
    for f in range(F):
        ok = bins[:, f] < B
        np.add.at(ones, (node[ok], f, bins[ok, f].astype(np.int64)), y[ok])
    lay = PackedLayout.for_sum(pk, 1, 0, n)
    packed, cnt = parallel_ops.histogram_packed(enc.encrypt_to_buffer(y), bins, B, lay, 1, node, nodes)
    assert packed.shape == (nodes, F, B) and packed.bound == int(cnt.max())
    assert np.asarray(dec.decrypt(packed)).reshape(nodes, F, B).tolist() == ones.tolist()
    # (g, h) of a sample in the two slots of one ciphertext
    gh = rng.integers(-1000, 1001, (n, 2)).astype(np.int64)
    lay2 = PackedLayout(pk, 32, 11, 0, 2)
    src = enc.encrypt_packed(gh, lay2)
    src.bound = 1000
    out, c2 = src.histogram(bins, B, node, nodes)
    want = np.zeros((nodes, F, B, 2), dtype=np.int64)
    for f in range(F):
        ok = bins[:, f] < B
        np.add.at(want, (node[ok], f, bins[ok, f].astype(np.int64)), gh[ok])
    assert np.array_equal(c2, cnt) and out.shape == (nodes, F, B, 2) and out.bound == 1000 * int(cnt.max())
    assert np.asarray(dec.decrypt(out)).reshape(nodes, F, B, 2).tolist() == want.tolist()
    # the overflow refusal fires before any launch
    calls = []
    monkeypatch.setattr(N.Context, "histogram", lambda *a, **k: calls.append(1))
    src.bound = lay2.slot_max // 2
    with pytest.raises(OverflowError):
        src.histogram(bins, B, node, nodes)
    assert not calls
