"""GPU parity of segmented weighted sums (pai_segment_dot: kernels_sd.hpp k_sd_sign, k_sd_gather, k_sd_acc over k_mm_tab's
tables, and the term path gather + k_mul + batch inversion + segmented add), bit-exact against the reference-generated
vectors (tests/golden/make_golden_segdot.py) and against the composition pai_mul over the gathered entries +
pai_segment_add on the same context.

The product library keeps small calls on the term path (flexpai.hip sd_take_fused); the shapes below reach the fused
kernels on the test build under $FLEXPAI_SD_ALWAYS=1 (the same object code in both libraries)."""
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (0, 1, 15, 16, 17, 33)          # neighbours in one wave: chains of 0, 1, 1, 1, 2 and 3 chunks, ragged last chunks
NCT = 40


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def gsd():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_segdot.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _always_fused(monkeypatch):
    monkeypatch.setenv("FLEXPAI_SD_ALWAYS", "1")          # read by the test build only, at every call
    monkeypatch.delenv("FLEXPAI_MM_TABLE_BYTES", raising=False)
    monkeypatch.delenv("FLEXPAI_SD_SLICE", raising=False)


@pytest.fixture(scope="module")
def ctxs(golden, xlib):
    N = _native()
    out = {}
    for nb in (1024, 2048, 4096):
        n = int(golden["keys"][str(nb)]["n"], 16)
        out[nb] = (N.Context(n, 0, lib=xlib), n)
    return out


@pytest.fixture(scope="module")
def operands(ctxs):
    """Per key size 40 random units mod n^2 as ciphertexts with exponents spread over 0 .. 20 (one at 25, the largest),
    shared by the cases below and never modified."""
    N = _native()
    out = {}
    for nb, (ctx, n) in ctxs.items():
        rng = np.random.default_rng(nb)
        cs = [int.from_bytes(rng.bytes(nb // 4), "little") % (n * n) for _ in range(NCT)]
        ex = rng.integers(0, 21, NCT).astype(np.int32)
        ex[7] = 25
        out[nb] = (N.ints_to_words(cs, ctx.ct_words), ex, cs)
    return out


def _case(dt, seed=1):
    """(index, seg_off, x): 82 entries in segments of LENS; negative scalars on the ciphertexts 0, 5, 10, .. only; an
    index repeated within a chunk, across the chunks of a segment and across segments; for floats +0.0, -0.0, a stored
    zero on the ciphertext with the largest exponent and a NaN."""
    rng = np.random.default_rng(seed)
    nnz = sum(LENS)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    idx = rng.integers(0, NCT, nnz).astype(np.int64)
    idx[2] = idx[3] = idx[1]                 # within the chunk of the 15-entry segment
    idx[49 + 20] = idx[49 + 2]               # across the chunks of the 33-entry segment
    idx[40] = idx[1]                         # across segments
    idx[20] = 7                              # the ciphertext at exponent 25, inside the 16-entry segment
    if dt == np.int64:
        x = rng.integers(1, 2 ** 40, nnz, dtype=np.int64)
        x[5] = 0
        x[20] = 0
    else:
        x = (np.abs(rng.standard_normal(nnz)) + 0.1) * 10.0 ** rng.integers(-6, 7, nnz)
        x[5], x[6], x[20] = 0.0, -0.0, 0.0
        x = x.astype(dt)
    x = np.where(idx % 5 == 0, -x, x)
    if dt != np.int64:
        x[6] = -0.0
        x[60] = np.nan
    return idx, off, x


def _compose(ctx, ct, ex, idx, off, x):
    """What exists without pai_segment_dot: pai_mul over the gathered entries, then pai_segment_add over ranges."""
    m, me, st = ctx.mul(ct[idx], ex[idx], x)
    out, oe = ctx.segment_add(m, me, np.arange(idx.size, dtype=np.int64), off)
    return out, oe, st


def _run(ctx, fused, *args):
    ctx.set_segdot_fused(fused)
    try:
        res = ctx.segment_dot(*args)
        assert ctx.segdot_path == (2 if fused else 1)
    finally:
        ctx.set_segdot_fused(True)
    return res


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_options_and_dispatch(golden):
    """The product library: option numbers, defaults, the read-only report; a small call stays on the term path."""
    N = _native()
    assert (N.PAI_OPT_SEGDOT_FUSED, N.PAI_OPT_SEGDOT_PATH) == (20, 21)
    n = int(golden["keys"]["1024"]["n"], 16)
    ctx = N.Context(n, 0)
    assert ctx.segdot_fused and ctx.segdot_path == 0
    rng = np.random.default_rng(3)
    ct = N.ints_to_words([int.from_bytes(rng.bytes(256), "little") % (n * n) for _ in range(4)], ctx.ct_words)
    ex = np.zeros(4, dtype=np.int32)
    out, oe, st = ctx.segment_dot(ct, ex, [0, 1, 2, 3, 3], [0, 2, 5], np.array([1.0, -2.0, 3.0, 0.5, 0.25]))
    assert ctx.segdot_path == 1 and not st.any()
    assert _same((out, oe), _compose(ctx, ct, ex, np.array([0, 1, 2, 3, 3]), np.array([0, 2, 5]),
                                     np.array([1.0, -2.0, 3.0, 0.5, 0.25]))[:2])
    # 65 536 entries over 4 ciphertexts: inside the dispatch's class; one entry fewer, or little reuse, is not
    idx = rng.integers(0, 4, 65536).astype(np.int64)
    off = np.arange(0, 65537, 64, dtype=np.int64)
    x = rng.standard_normal(65536)
    a = ctx.segment_dot(ct, ex, idx, off, x)
    assert ctx.segdot_path == 2
    ctx.segment_dot(ct, ex, idx[:-1], np.append(off[:-1], 65535), x[:-1])
    assert ctx.segdot_path == 1
    ctx.set_segdot_fused(False)
    assert not ctx.segdot_fused
    b = ctx.segment_dot(ct, ex, idx, off, x)
    assert ctx.segdot_path == 1 and _same(a, b)
    assert ctx.lib.pai_ctx_set_option(ctx.handle, N.PAI_OPT_SEGDOT_PATH, 1) != 0   # read-only


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("nb", [1024, 2048])
def test_reference_golden(ctxs, gsd, nb, fused):
    N = _native()
    ctx, _ = ctxs[nb]
    g = gsd["cases"][str(nb)]
    ct = N.ints_to_words([int(h, 16) for h in g["c"]], ctx.ct_words)
    ex = np.array(g["e"], dtype=np.int32)
    for name in ("f64", "i64"):
        w = (np.array([float.fromhex(v) for v in g["weights"][name]]) if name == "f64"
             else np.array(g["weights"][name], dtype=np.int64))
        out, oe, st = _run(ctx, fused, ct, ex, g["index"], g["seg_off"], w)
        assert not st.any()
        want = [(1, -(1 << 31)) if v is None else (int(v[0], 16), v[1]) for v in g["out"][name]]
        assert list(zip(N.words_to_ints(out), (int(e) for e in oe))) == want


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.int64])
@pytest.mark.parametrize("nb", [1024, 2048])
def test_equals_mul_plus_segment_add(ctxs, operands, nb, dt):
    N = _native()
    ctx, _ = ctxs[nb]
    ct, ex, _ = operands[nb]
    idx, off, x = _case(dt)
    want = _compose(ctx, ct, ex, idx, off, x)
    if dt != np.int64:
        assert want[2][60] == N.EL_ENC_RANGE and np.count_nonzero(want[2]) == 1      # the NaN, and only it
    else:
        assert not want[2].any()
    assert N.words_to_ints(want[0][:1]) == [1] and want[1][0] == -(1 << 31)          # the empty segment
    assert want[1][3] == 25 + 0 if dt == np.int64 else want[1][3] >= 25            # the stored zero holds the maximum
    for fused in (True, False):
        assert _same(_run(ctx, fused, ct, ex, idx, off, x), want), fused


def test_4096_bits(ctxs, operands):
    ctx, _ = ctxs[4096]
    ct, ex, _ = operands[4096]
    rng = np.random.default_rng(4096)
    idx = rng.integers(0, NCT, 20).astype(np.int64)
    off = np.array([0, 3, 3, 20], dtype=np.int64)
    x = rng.standard_normal(20) * 10.0 ** rng.integers(-3, 4, 20)
    want = _compose(ctx, ct, ex, idx, off, x)
    for fused in (True, False):
        assert _same(_run(ctx, fused, ct, ex, idx, off, x), want), fused


def test_blocks_and_slices_keep_the_bits(ctxs, operands, monkeypatch):
    """A table budget of 16 ciphertexts with both signs: every chunk of 16 distinct ciphertexts is a block of its own, so
    the call takes at least 3 blocks and the 33-entry segment (chunks of 16, 16 and 1) is cut between them. The term
    path in slices of 2 chunks cuts it as well."""
    ctx, _ = ctxs[1024]
    ct, ex, _ = operands[1024]
    idx, off, x = _case(np.float64, seed=2)
    want = _run(ctx, True, ct, ex, idx, off, x)
    assert _same(want, _compose(ctx, ct, ex, idx, off, x))
    monkeypatch.setenv("FLEXPAI_MM_TABLE_BYTES", str(16 * 2 * 16 * 74 * 4))         # 16 rows of S = 74 limbs, two signs
    assert _same(_run(ctx, True, ct, ex, idx, off, x), want)
    monkeypatch.setenv("FLEXPAI_MM_TABLE_BYTES", str(1))                            # one chunk per block
    assert _same(_run(ctx, True, ct, ex, idx, off, x), want)
    monkeypatch.setenv("FLEXPAI_SD_SLICE", "2")
    assert _same(_run(ctx, False, ct, ex, idx, off, x), want)


def test_errors(ctxs, operands, golden):
    N = _native()
    ctx, n = ctxs[1024]
    ct, ex, cs = operands[1024]
    x = np.ones(3)
    lib = ctx.lib

    def rc(idx, off, nseg):
        idx, off = np.array(idx, dtype=np.int64), np.array(off, dtype=np.int64)
        out = np.empty((nseg, ctx.ct_words), dtype=np.uint32)
        oe = np.empty(nseg, dtype=np.int32)
        return lib.pai_segment_dot(ctx.handle, ct.ctypes.data, ex.ctypes.data, NCT, idx.ctypes.data, off.ctypes.data, nseg,
                                   N.PAI_F64, x.ctypes.data, out.ctypes.data, oe.ctypes.data, None)

    assert rc([0, 1, 2], [0, 3], 1) == 0
    assert rc([0, NCT, 2], [0, 3], 1) == -1
    assert rc([0, -1, 2], [0, 3], 1) == -1
    assert rc([0, 1, 2], [0, 2, 1, 3], 3) == -1
    assert rc([0, 1, 2], [1, 3], 1) == -1
    # a multiple of p: fine under positive scalars, no inverse under a negative one, on both paths
    p = int(golden["keys"]["1024"]["p"], 16)
    bad = N.ints_to_words(cs[:4] + [p * 12345], ctx.ct_words)
    idx, off = np.array([0, 4, 2, 4], dtype=np.int64), np.array([0, 2, 4], dtype=np.int64)
    for fused in (True, False):
        got = _run(ctx, fused, bad, ex[:5], idx, off, np.array([1.0, 2.0, -3.0, 4.0]))
        assert _same(got, _compose(ctx, bad, ex[:5], idx, off, np.array([1.0, 2.0, -3.0, 4.0])))
        ctx.set_segdot_fused(fused)
        try:
            with pytest.raises(ZeroDivisionError):
                ctx.segment_dot(bad, ex[:5], idx, off, np.array([1.0, 2.0, 3.0, -4.0]))
        finally:
            ctx.set_segdot_fused(True)


@pytest.mark.parametrize("fused", [False, True])
def test_dev_variant_on_a_stream(ctxs, operands, fused):
    import torch
    N = _native()
    ctx, _ = ctxs[1024]
    ct, ex, _ = operands[1024]
    idx, off, x = _case(np.float64, seed=3)
    want = _run(ctx, fused, ct, ex, idx, off, x)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_ct = torch.from_numpy(ct.view(np.int32)).to(dev)
        d_ex = torch.from_numpy(ex).to(dev)
        d_x = torch.from_numpy(x).to(dev)
        d_out = torch.empty((len(LENS), ctx.ct_words), dtype=torch.int32, device=dev)
        d_oe = torch.empty(len(LENS), dtype=torch.int32, device=dev)
        d_st = torch.empty(idx.size, dtype=torch.int32, device=dev)
        ctx.set_segdot_fused(fused)
        try:
            rc = ctx.lib.pai_segment_dot_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), NCT, idx.ctypes.data,
                                             off.ctypes.data, len(LENS), N.PAI_F64, d_x.data_ptr(), d_out.data_ptr(),
                                             d_oe.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        finally:
            ctx.set_segdot_fused(True)
        assert rc == 0, ctx.lib.pai_last_error().decode()
        assert ctx.segdot_path == (2 if fused else 1)
        stream.synchronize()
    got = (d_out.cpu().numpy().view(np.uint32), d_oe.cpu().numpy(), d_st.cpu().numpy())
    assert _same(got, want)


def test_package_sparse_dot_and_parallel_ops():
    """buf.dot(csc) against the dense product in decrypted values (the dense product also counts the absent zeros'
    exponents, so its bits may differ; both decode the same rational, each with one rounding to double: rtol 1e-13),
    and in bits against segment_dot over the same entries; the object-array route through parallel_ops.segment_dot
    against the per-object operators."""
    import scipy.sparse as sp
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    pe, pd = generate_paillier_encryptor_decryptor(1024, seed=5)
    rng = np.random.default_rng(12)
    m, K, d = 2, 12, 5
    v = rng.standard_normal((m, K))
    enc = pe.encrypt(v)
    buf = CiphertextBuffer.from_array(enc)
    dense = rng.standard_normal((K, d)) * (rng.random((K, d)) < 0.4)
    dense[:, 3] = 0.0                                      # an empty column
    csc = sp.csc_matrix(dense)
    got = buf.dot(csc)
    assert got.shape == (m, d)
    assert np.allclose(pd.decrypt(got), pd.decrypt(buf.dot(dense)), rtol=1e-13, atol=0)
    assert np.allclose(pd.decrypt(got), v.dot(dense), rtol=1e-9, atol=1e-12)
    row0 = buf.reshape(m * K).segment_dot(csc.indices, csc.indptr, csc.data)
    assert np.array_equal(row0.words, got.words[:d]) and np.array_equal(row0.exps, got.exps[:d])
    arr = enc @ csc
    assert arr.shape == (m, d) and np.array_equal(CiphertextBuffer.from_array(arr).words, got.words)
    objs = np.asarray(enc).reshape(-1)
    lists = [[0, 5, 5], [], [23, -1]]
    weights = [np.array([1.5, -2.0, 0.0]), np.array([]), np.array([3.0, 4.0])]
    res = parallel_ops.segment_dot(objs, lists, weights)
    want = [sum(objs[i] * float(w) for i, w in zip(idx, ws)) for idx, ws in zip(lists, weights)]
    assert res[1] == 0
    for a, b in ((res[0], want[0]), (res[2], want[2])):
        assert (a.ciphertext(False), a.exponent) == (b.ciphertext(False), b.exponent)
