"""The uneven digit cut of the key holder's fixed-base exponent (csrc/fb_cut.hpp) on the GPU: under a memory budget that
only lets a window W below the asked one through, the Shoup-row tables take K - 1 digits, the first few one bit wider,
instead of the uniform cut's K -- and not one ciphertext bit moves, because a_h is reduced mod p_h - 1 before it is cut.

Smallest shapes that can still go wrong: base windows 8 (1024 = 128 x 8 has no short digit: 8 digits of 9 bits and 119
of 8; LO = 4 for both widths) and 12 (1024 = 85 x 12 + 4: 4 digits of 13 bits, LO = 6, HI = 7 against 6), at nb = 1024
(S = 19) and 2048 (S = 37); 300 and 129 elements (ragged against the 128-pair block, and one element past it). Each
case runs on the product library and on the guard build, where every digit, row index and table store formed from the
new offsets is range-checked (csrc/guard.hpp): a violation fails the call."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

ROW_BYTES = {1024: 224, 2048: 448}
ASKED = {8: 12, 12: 16}          # the window asked for, one ladder step above the base window the budget allows
RK = bytes(range(60, 92))


def _key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _cut_bytes(kb, K, row):
    """Both halves' tables of the K-digit cut with the fewest rows: kb mod K digits of kb // K + 1 bits, the rest of kb // K."""
    w, nw = divmod(kb, K)
    return 2 * (nw * (2 << w) + (K - nw) * (1 << w)) * row


def _run(N, lib, key, asked, budget, monkeypatch, golden_fb, nb):
    monkeypatch.setenv("FLEXPAI_FB_MAX_BYTES", str(budget))
    ctx = N.Context(key.n, 0, key.p, key.q, **({"lib": lib} if lib is not None else {}))
    try:
        ctx.set_fb_window(asked)
        ctx.prepare_fixed_base()
        assert ctx.split_sampler & 4
        info, nbytes = ctx.fixed_base_info(), ctx.fixed_base_setup()[2]
        outs = []
        for count, base in ((300, 2 ** 33 + 7), (129, 41)):
            x = (np.random.default_rng(count).standard_normal(count) * 1000).astype(np.float32)
            x[::11] = 0.0
            x[3::17] *= -1e6
            ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=base)
            assert np.all(st == 0)
            got = N.words_to_ints(ct)
            for i in sorted({0, 127, 128, count - 1}):
                assert (got[i], int(ex[i])) == O.fb_encrypt_value(x[i], key, RK, base + i, info[:2]), (count, i)
            val, _, _, _ = ctx.decrypt(ct, ex)
            assert np.array_equal(val, x.astype(np.float64))
            outs.append((ct, ex))
        recs = golden_fb["encrypt"][str(nb)]   # the reference's own ciphertexts under the sampler's obfuscator
        xg = np.array([r["bits"] for r in recs], dtype=np.uint32).view(np.float32)
        ct, ex, _ = ctx.encrypt(xg, obf_mode=N.PAI_OBF_RNG, rng_key=bytes.fromhex(golden_fb["rng_key"]),
                                index_base=golden_fb["index_base"])
        assert [(hex(c), int(e)) for c, e in zip(N.words_to_ints(ct), ex)] == [(r["c"], r["e"]) for r in recs]
        return info, nbytes, outs
    finally:
        ctx.close()


@pytest.mark.parametrize("guarded", [False, True], ids=["product", "guard"])
@pytest.mark.parametrize("nb,W", [(1024, 8), (2048, 8), (1024, 12), (2048, 12)])
def test_uneven_cut_is_bit_identical_to_the_uniform_cut(golden, golden_fb, xlib, monkeypatch, nb, W, guarded):
    from flex.crypto.paillier import _native as N
    key = _key(golden, nb)
    kb = max((key.p - 1).bit_length(), (key.q - 1).bit_length())
    assert kb == nb // 2
    row, Ku = ROW_BYTES[nb], -(-kb // W)
    uniform_bytes, uneven_bytes = 2 * Ku * (1 << W) * row, _cut_bytes(kb, Ku - 1, row)
    assert uniform_bytes < uneven_bytes < 2 * -(-kb // ASKED[W]) * (1 << ASKED[W]) * row
    lib = xlib if guarded else None
    # a budget of exactly the uniform tables: no cut with fewer digits fits, the plan is the uniform one
    (gp, gq, K0, W0), bytes0, outs0 = _run(N, lib, key, ASKED[W], uniform_bytes, monkeypatch, golden_fb, nb)
    assert (K0, W0, bytes0) == (Ku, W, uniform_bytes)
    # ... one byte short of the uneven cut's tables: still the uniform plan
    monkeypatch.setenv("FLEXPAI_FB_MAX_BYTES", str(uneven_bytes - 1))
    ctx = N.Context(key.n, 0, key.p, key.q, **({"lib": lib} if guarded else {}))
    try:
        ctx.set_fb_window(ASKED[W])
        assert ctx.fixed_base_info()[2:] == (Ku, W) and ctx.fixed_base_setup()[2] == uniform_bytes
    finally:
        ctx.close()
    # ... exactly the uneven cut's tables: one digit fewer, the base width reported as the window, the true bytes
    (gp1, gq1, K1, W1), bytes1, outs1 = _run(N, lib, key, ASKED[W], uneven_bytes, monkeypatch, golden_fb, nb)
    assert (gp1, gq1) == (gp, gq)
    assert (K1, W1, bytes1) == (Ku - 1, W, uneven_bytes)
    for (a, ea), (b, eb) in zip(outs0, outs1):
        assert np.array_equal(a, b) and np.array_equal(ea, eb)
