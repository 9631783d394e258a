"""GPU parity of encrypted histograms over C ciphertext columns (pai_histogram_cols[_dev]: k_hist_acc_c over (run,
column) items, k_hist_seg_cols, the device-planned segmented add) against Python integers, bit for bit, through the
host call, the device call and DeviceCiphertextBuffer.histogram."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = -(1 << 31)
F, B, NODES = 3, 4, 2
SIZES = ((0, 0, 1), (0, 1, 63), (0, 2, 64), (1, 0, 65), (1, 1, 129))   # (node, bin of feature 0, members): HIST_RUN seams


def _native():
    from flex.crypto.paillier import _native as N
    return N


@functools.lru_cache(maxsize=None)
def modulus(nb):
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        return int(json.load(f)["keys"][str(nb)]["n"], 16)


@functools.lru_cache(maxsize=None)
def case(nb, C, small=False):
    """(ciphertexts [N][C], exponents [N, C], bins [N, F + 2] with two unused columns, node [N], expected cells
    {(v, f, b): [(value, E)] * C}): feature 0 has cells of 1, 63, 64, 65 and 129 members and empty ones (bin 3, and node
    1 from bin 2 on), node ids -1 and NODES, one bin id >= B; the exponents differ between columns and members."""
    nsq = modulus(nb) ** 2
    rng = np.random.default_rng(nb + C)
    node = np.concatenate([np.full(m, v) for v, _, m in SIZES] + [[-1, -1, NODES, NODES, 0]]).astype(np.int32)
    bin0 = np.concatenate([np.full(m, b) for _, b, m in SIZES] + [[0, 1, 0, 1, B]])
    if small:
        node, bin0 = node[-200:], bin0[-200:]
    n = node.size
    order = rng.permutation(n)
    node, bin0 = node[order], bin0[order]
    bins = rng.integers(0, B + 1, (n, F + 2))
    bins[:, 0] = bin0
    exps = rng.integers(0, 4, (n, C)).astype(np.int32)
    cts = [[int.from_bytes(rng.bytes(nb // 4), "little") % nsq for _ in range(C)] for _ in range(n)]
    for i in range(0, n, 7):
        cts[i][0] = nsq - 1 - i                                # near n^2 - 1 in one column
    want = {}
    for v in range(NODES):
        for f in range(F):
            for b in range(B):
                mem = np.flatnonzero((node == v) & (bins[:, f] == b)).tolist()
                cols = []
                for c in range(C):
                    E = max((int(exps[i, c]) for i in mem), default=EMPTY)
                    acc = 1
                    for i in mem:
                        acc = acc * pow(cts[i][c], 16 ** (E - int(exps[i, c])), nsq) % nsq
                    cols.append((acc, E))
                want[v, f, b] = (len(mem), cols)
    return cts, exps, bins, node, want


def check(out_ints, oe, cnt, want, C):
    for (v, f, b), (members, cols) in want.items():
        s = (v * F + f) * B + b
        assert cnt[s] == members, (v, f, b)
        for c in range(C):
            assert (out_ints[s * C + c], int(oe[s * C + c])) == cols[c], (v, f, b, c)


def run_all_routes(nb, C, dtype, small=False):
    import torch
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.device_buffer import device_array
    from flex.crypto.paillier.keypair import PaillierPublicKey
    N = _native()
    cts, exps, bins, node, want = case(nb, C, small)
    sizes = sorted(m for m, _ in want.values())
    assert sizes[0] == 0 and (small or {1, 63, 64, 65, 129} <= set(sizes))
    n = node.size
    ctx = N.Context(modulus(nb), 0)
    W = ctx.ct_words
    words = N.ints_to_words([x for row in cts for x in row], W)
    wide = bins.astype(dtype)
    cells = NODES * F * B
    # the host call, strided bins
    out, oe, cnt = ctx.histogram(words, exps.reshape(-1), wide[:, :F], B, node, NODES, cols=C)
    check(N.words_to_ints(out), oe, cnt, want, C)
    # the device call
    dev = torch.device("cuda", 0)
    d_ct = torch.from_numpy(words.view(np.int32)).to(dev)
    d_ex = torch.from_numpy(exps).to(dev)
    d_bins = torch.from_numpy(wide.view(np.int8 if dtype == np.uint8 else np.int16)).to(dev)
    d_node = torch.from_numpy(node).to(dev)
    d_out = torch.empty((cells * C, W), dtype=torch.int32, device=dev)
    d_oe = torch.empty(cells * C, dtype=torch.int32, device=dev)
    d_cnt = torch.empty(cells, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rc = ctx.lib.pai_histogram_cols_dev(ctx.handle, d_ct.data_ptr(), d_ex.data_ptr(), n, C,
                                        N.PAI_BIN_U16 if dtype == np.uint16 else N.PAI_BIN_U8, d_bins.data_ptr(), F, F + 2,
                                        d_node.data_ptr(), NODES, B, d_out.data_ptr(), d_oe.data_ptr(), d_cnt.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out)
    assert np.array_equal(d_oe.cpu().numpy(), oe) and np.array_equal(d_cnt.cpu().numpy(), cnt)
    # the resident buffer, resident bins and node ids
    if C > 1:
        buf = CiphertextBuffer(PaillierPublicKey(modulus(nb)), words, exps.reshape(-1), None, (n, C)).to_device()
        hist, counts = buf.histogram(device_array(np.ascontiguousarray(wide[:, :F])), B, node=device_array(node), n_nodes=NODES)
        assert hist.shape == (NODES, F, B, C) and counts.shape == (NODES, F, B)
        host = hist.to_host()
        assert np.array_equal(host.words, out) and np.array_equal(counts.reshape(-1), cnt)
        assert np.array_equal(host.exps, np.where(np.repeat(cnt, C) == 0, 0, oe))
    return ctx, words, exps, wide, node, (out, oe, cnt)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("C", [1, 2, 3, 5])
@pytest.mark.parametrize("nb", [1024, 2048])
def test_parity_with_python_integers(nb, C, dtype):
    run_all_routes(nb, C, dtype)


def test_parity_4096():
    run_all_routes(4096, 2, np.uint8, small=True)


@pytest.mark.parametrize("C", [1, 3])
def test_columns_equal_pai_histogram(C):
    """Column c has the bits of pai_histogram on the contiguous copy of column c (C = 1: the same buffers)."""
    ctx, words, exps, wide, node, (out, oe, cnt) = run_all_routes(1024, C, np.uint8)
    W = ctx.ct_words
    for c in range(C):
        w1, e1, c1 = ctx.histogram(np.ascontiguousarray(words.reshape(-1, C, W)[:, c]), np.ascontiguousarray(exps[:, c]),
                                   wide[:, :F], B, node, NODES)
        assert np.array_equal(out.reshape(-1, C, W)[:, c], w1) and np.array_equal(oe.reshape(-1, C)[:, c], e1)
        assert np.array_equal(cnt, c1)


def test_argument_errors():
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    N = _native()
    ctx = N.Context(modulus(1024), 0)
    cts, exps, bins, node, _ = case(1024, 2)
    words = N.ints_to_words([x for row in cts for x in row], ctx.ct_words)
    e, b8 = exps.reshape(-1), np.ascontiguousarray(bins[:, :F].astype(np.uint8))
    out = np.empty((4, ctx.ct_words), dtype=np.uint32)

    def call(C, nodes=NODES, n=node.size):
        return ctx.lib.pai_histogram_cols(ctx.handle, words.ctypes.data, e.ctypes.data, n, C, N.PAI_BIN_U8, b8.ctypes.data, F, F,
                                          node.ctypes.data, nodes, B, out.ctypes.data, out.ctypes.data, None)
    assert call(0) == -1                                       # C = 0
    assert call(2, nodes=(1 << 23) // (F * B) + 1) == -1       # nodes F B <= 2^24 < nodes F B C
    assert call(1 << 20, n=1 << 11) == -1                      # N C = 2^31

    class Sparse:                                              # anything that offers .tocsr() is sparse
        shape = (node.size, F)

        def tocsr(self):
            raise AssertionError("a sparse operand must be refused before it is read")
    buf = CiphertextBuffer(PaillierPublicKey(modulus(1024)), words, e, None, (node.size, 2))
    for operand in (buf, buf.to_device()):
        with pytest.raises(TypeError):
            operand.histogram(Sparse(), B, node=node, n_nodes=NODES)
