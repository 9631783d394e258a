"""k_modinv (csrc/kernels_inv.hpp) and what is built on it, against Python's pow(x, -1, m) and the oracle's invert:
pai_debug_modinv over the widths at which the layout changes (one to four words per lane, ragged last lane), pai_neg /
pai_neg_dev / -buf, PAI_OPT_INV_DEVICE 0 against 1, and pai_encrypt_dev's public-key chain on two streams."""
import math
import random

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
INV_TOPS = 64
FILL = 0xA5A5A5A5


def _native():
    from flex.crypto.paillier import _native
    return _native


def _key(golden, nb):
    if nb == 3072:
        from flex.crypto.paillier import _bigint
        rng = random.Random(3072)
        p, q = (_bigint.next_prime(rng.getrandbits(1536) | 1 << 1535 | 1 << 1534) for _ in range(2))
        return O.Key(p * q, p, q)
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _moduli(W, golden):
    rng = random.Random(1000 + W)
    top = 1 << (32 * W - 1)
    ms = [rng.getrandbits(32 * W) | top | 1, (1 << 32 * W) - 19, top + 1,
          (1 << 32 * (W - 1)) | rng.getrandbits(32 * (W - 1)) | 1]
    if W in (64, 128, 192, 256):
        ms.append(_key(golden, 16 * W).nsquare)
    return ms


def _residues(m, W, rng):
    K = (W + 63) // 64
    xs = [1, 2, m - 1, m - 2, (m + 1) // 2]
    for j in (31, 32, 63, 64, 32 * K - 1, 32 * K + 1):
        xs += [1 << j, m - (1 << j)]
    f0, f1 = 1, 2
    while f0 + f1 < m:
        f0, f1 = f1, f0 + f1
    xs += [rng.getrandbits(32) | 1, rng.getrandbits(max(32 * (W - 1), 1)), f0, f1, 0, 0, 0]
    xs += [rng.randrange(m) for _ in range(43)]
    return [x % m for x in xs]                      # 67: two blocks' worth of waves and a ragged rest; the zeros have no inverse


def _check(xs, m, W, tag):
    """status 0 and pow(x, -1, m) where there is an inverse; status 1 and the row's fill pattern where there is none"""
    N = _native()
    out, st = N.modinv(xs, m, W, FILL)
    got, fill = N.words_to_ints(out), int.from_bytes(b"\xa5" * 4 * W, "little")
    for i, x in enumerate(xs):
        unit = math.gcd(x, m) == 1
        assert st[i] == (0 if unit else 1) and got[i] == (pow(x, -1, m) if unit else fill), (tag, i, hex(x))


@pytest.mark.parametrize("W", [1, 2, 33, 64, 65, 128, 192, 256])
def test_modinv_against_pow(W, golden):
    for mi, m in enumerate(_moduli(W, golden)):
        _check(_residues(m, W, random.Random(7 * W + mi)), m, W, (W, mi))


@pytest.mark.parametrize("W", [2, 64, 130])
def test_modinv_no_inverse_statuses(W):
    p = 0xFFFFFFFB                                  # prime
    c = random.Random(W).getrandbits(32 * W - 40) | 1
    m = p * c
    xs = [3, 0, p, 5, m // p, 2 * p, 7, c * 3 % m, m - 1]
    assert all(math.gcd(xs[i], m) > 1 for i in (1, 2, 4, 5, 7)) and math.gcd(m - 1, m) == 1
    _check(xs, m, W, W)


def _random_cts(key, count, seed):
    return [random.Random(seed + i).randrange(1, key.nsquare) for i in range(count)]


# levels (segments of 4 up to 16384 values, stop at <= 64): 1, 64, 65 one; 4096 -> 1024 -> 256 -> 64 three; 4097 four
@pytest.mark.parametrize("nb", [1024, 2048, 3072, 4096])
def test_neg_matches_oracle_invert(golden, nb):
    N = _native()
    key = _key(golden, nb)
    ctx = N.Context(key.n, 0, key.p, key.q)
    W = ctx.ct_words
    cs = _random_cts(key, 130, nb)
    base, want = N.ints_to_words(cs, W), N.ints_to_words([O.mul_scalar(c, 0, -1, key)[0] for c in cs], W)
    s = N.DeviceMem(4, 0)

    def neg_dev(words, expect, status):                 # out of place, then in place
        d, o = N.device_upload(words, 0), N.device_upload(np.full_like(words, FILL), 0)
        for dst in (o, d):
            ctx.dev_call("pai_neg_dev", d.ptr, len(words), dst.ptr, s.ptr)
            assert s.download(np.uint32, 1)[0] == status
            assert np.array_equal(dst.download(np.uint32, words.size).reshape(words.shape), expect), (nb, len(words))

    for count in (1, INV_TOPS, INV_TOPS + 1, 4096, 4097):
        reps = -(-count // len(cs))
        words, want_w = np.tile(base, (reps, 1))[:count], np.tile(want, (reps, 1))[:count]
        assert np.array_equal(ctx.neg(words), want_w), (nb, count)
        neg_dev(words, want_w, 0)
    if nb != 1024:
        return
    # -buf on both buffer classes is * -1, exponents included
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    buf = CiphertextBuffer(PaillierPublicKey(key.n), base, np.arange(130, dtype=np.int32) - 30, 0, (130,))
    for got in (-buf, (-buf.to_device()).to_host()):
        assert np.array_equal(got.words, want) and np.array_equal(got.exps, (buf * -1).exps)
    # one multiple of p: the status word is set, nothing but the out-of-place copy is written, the host call raises
    bad = base.copy()
    bad[77] = N.ints_to_words([12345 * key.p], W)[0]
    with pytest.raises(ZeroDivisionError):
        ctx.neg(bad)
    neg_dev(bad, bad, 1)


def test_inv_device_option_same_bits(golden, xlib, monkeypatch):
    """pai_mul_dev with mixed-sign scalars, one fused matmul with negative entries (the test build under
    FLEXPAI_MM_ALWAYS=1, as tests/test_gpu_mm.py) and one sparse histogram with default cells: PAI_OPT_INV_DEVICE = 0
    (host step) and 1 (k_modinv) give identical words."""
    import scipy.sparse as sp
    monkeypatch.setenv("FLEXPAI_MM_ALWAYS", "1")
    N = _native()
    key = _key(golden, 1024)
    ctx = N.Context(key.n, 0, key.p, key.q, lib=xlib)
    pctx = N.Context(key.n, 0)
    W = ctx.ct_words
    rng = np.random.default_rng(3)
    cs = N.ints_to_words(_random_cts(key, 330, 11), W)
    exps = rng.integers(-8, 8, 330).astype(np.int32)
    x, xm = rng.standard_normal(330) * 100, rng.integers(-5, 6, (33, 2)).astype(np.float64)
    csr = sp.csr_matrix(rng.integers(0, 3, (40, 2)))
    d_ct, d_ex, d_x = (N.device_upload(v, 0) for v in (cs, exps, x))
    out, oe, st = N.DeviceMem(330 * W * 4, 0), N.DeviceMem(330 * 4, 0), N.DeviceMem(330 * 4, 0)
    got = {}
    for on in (0, 1):
        for c in (ctx, pctx):
            c.set_inv_device(bool(on))
        pctx.dev_call("pai_mul_dev", d_ct.ptr, d_ex.ptr, 330, N.PAI_F64, d_x.ptr, 1, out.ptr, oe.ptr, st.ptr)
        r = [(out.download(np.uint32, 330 * W), oe.download(np.int32, 330)), ctx.matmul(cs[:99], exps[:99], 3, 33, xm, 2)]
        assert ctx.matmul_path == 2
        r.append(pctx.histogram_sparse(cs[:40], exps[:40], csr.indptr, csr.indices, csr.data.astype(np.uint8), 2,
                                       np.zeros(2, dtype=np.int32), 3)[:2])
        got[on] = r
    for a, b in zip(got[0], got[1]):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_public_chain_on_two_streams(golden):
    """pai_encrypt_dev's factored public-key chain (chunks of >= 16384 elements, batch inversion mod n) on two streams of
    one context, interleaved, against the same two calls made one after the other on the null stream."""
    import torch
    N = _native()
    ctx = N.Context(_key(golden, 2048).n, 0)
    n_el, W = 16384, ctx.ct_words
    calls = [(N.device_upload(np.linspace(-3, 3 + i, n_el).astype(np.float32), 0), bytes(range(i, 32 + i))) for i in (0, 1)]

    def run(streams):
        outs = [N.DeviceMem(n_el * W * 4, 0) for _ in calls]
        ex, ss = N.DeviceMem(n_el * 4, 0), N.DeviceMem(n_el * 4, 0)
        for (dx, k), ct, st in zip(calls, outs, streams):
            ctx._chk(ctx.lib.pai_encrypt_dev(ctx._h, N.PAI_F32, dx.ptr, n_el, 0, 0, N.PAI_OBF_RNG, None, 0, 0, k, 7,
                                             ct.ptr, ex.ptr, ss.ptr, st))
        torch.cuda.synchronize()
        return [ct.download(np.uint32, n_el * W) for ct in outs]

    for a, b in zip(run([None, None]), run([torch.cuda.Stream().cuda_stream, torch.cuda.Stream().cuda_stream])):
        assert np.array_equal(a, b)
