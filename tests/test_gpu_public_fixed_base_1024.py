"""GPU parity of the 1024-bit public fixed-base sampler (kernels_pfb1.hpp: k_pfb1, PAI_OPT_PUBLIC_FB = 2) against the
oracle's restatement of the reference's ciphertext under the sampler's r (oracle/paillier_oracle.py pfb_*), at the two
edges of its key range (tests/golden/pfb1_keys.json: n of 1024 bits with its top limb all ones, n of 1009 bits); the
same r^n on pai_obfuscate; and the default option value, which leaves such a context on k_pe1_* with no tables."""
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

RK = bytes(range(60, 92))


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(os.path.dirname(__file__), "golden", "pfb1_keys.json")) as f:
        ks = json.load(f)["keys"]
    return {name: (O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16)), [int(b, 16) for b in k["bases"]])
            for name, k in ks.items()}


@pytest.fixture(scope="module", params=[(name, w) for name in ("1024_top_limb_full", "1009") for w in (12, 16)],
                ids=lambda p: f"{p[0]}-W{p[1]}")
def sampler(request, keys):
    """A public-only context with the sampler opted in, the golden bases and resident tables at one window."""
    key, bases = keys[request.param[0]]
    ctx = _native().Context(key.n, 0)
    ctx.set_public_fixed_base(2)
    ctx.set_public_bases(bases)
    ctx.set_pfb_window(request.param[1])
    ctx.prepare_public_fixed_base()
    yield ctx, key, bases, request.param[1]
    ctx.close()


@pytest.mark.parametrize("index_base", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("count", [1, 65, 300])
def test_encrypt_matches_oracle(sampler, count, index_base):
    N = _native()
    ctx, key, bases, window = sampler
    assert ctx.pfb_ready
    gb, K, W, K0 = ctx.public_fixed_base_info()
    assert gb == bases and W == window and (K0, (K - K0) // O.PFB_SHORT) == O.pfb_layout(key.n.bit_length(), window)
    x = (np.random.default_rng(count).standard_normal(count) * 100).astype(np.float32)
    x[0] = 0.0
    x[-1] = -3.25
    ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=index_base)
    assert np.all(st == 0)
    got = N.words_to_ints(ct)
    # every element up to one past a wave (index_base + i crosses 2^32 at i = 3); past that the wave and block seams, the
    # last element and every seventh between (the oracle's two exponentiations per element are the test's time)
    for i in sorted(i for i in set(range(66)) | {255, 256, 257, count - 1} | set(range(66, count, 7)) if i < count):
        assert (got[i], int(ex[i])) == O.pfb_encrypt_value(x[i], key, bases, RK, index_base + i, window), f"element {i}"


def test_obfuscate_draws_the_same_r(keys):
    """pai_obfuscate multiplies by the r^n that pai_encrypt of zeros gives at the same key and indices."""
    N = _native()
    key, bases = keys["1024_top_limb_full"]
    ctx = N.Context(key.n, 0)
    try:
        ctx.set_public_fixed_base(2)
        ctx.set_public_bases(bases)
        ctx.set_pfb_window(12)
        ctx.prepare_public_fixed_base()
        x = np.arange(1, 66, dtype=np.float32) * -1.5
        ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=[3 + i for i in range(65)])
        e0, _, _ = ctx.encrypt(np.zeros(65, dtype=np.float32), obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=2 ** 32 - 3)
        out = ctx.obfuscate(ct, rng_key=RK, index_base=2 ** 32 - 3)
        want = [c * e % key.nsquare for c, e in zip(N.words_to_ints(ct), N.words_to_ints(e0))]
        assert N.words_to_ints(out) == want
    finally:
        ctx.close()


def test_break_even_follows_the_measured_model(keys, monkeypatch):
    """Opted in and unprepared, a context builds its tables only past the measured break-even (profiles/pfb1_rate.json:
    build 0.067 s + 0.88 ns per row, 1/4.43 M - 1/15.3 M s saved per element at W = 16); a call below it stays on k_pe1_*."""
    monkeypatch.delenv("FLEXPAI_PFB_MIN_ELEMS", raising=False)
    key, _ = keys["1009"]
    ctx = _native().Context(key.n, 0)
    try:
        ctx.set_public_fixed_base(2)
        K0, KS = O.pfb_layout(1009, 16)
        want = int((0.067 + ((K0 + O.PFB_SHORT * KS) << 16) * 0.88e-9) / (1 / 4.43e6 - 1 / 15.3e6)) + 1
        assert abs(ctx.public_fixed_base_policy()[1] - want) <= 1 and 450_000 < want < 550_000
        ctx.encrypt(np.ones(65, dtype=np.float32), obf_mode=_native().PAI_OBF_RNG, rng_key=RK)
        assert not ctx.pfb_ready and ctx.public_fixed_base_policy()[0] == 65
    finally:
        ctx.close()


def test_default_option_keeps_the_per_element_chain(keys):
    """PAI_OPT_PUBLIC_FB = 1 (the default): no tables at 1024 bits, and the ChaCha20-r ciphertexts of k_pe1_*."""
    N = _native()
    key, bases = keys["1024_top_limb_full"]
    ctx = N.Context(key.n, 0)
    try:
        ctx.set_public_bases(bases)
        ctx.set_pfb_window(12)
        with pytest.raises(RuntimeError):
            ctx.prepare_public_fixed_base()
        x = (np.random.default_rng(65).standard_normal(65) * 100).astype(np.float32)
        ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=9)
        assert not ctx.pfb_ready
        got = N.words_to_ints(ct)
        rbytes = ((key.n.bit_length() + 64 + 31) // 32) * 4
        for i in range(65):
            assert (got[i], int(ex[i])) == O.encrypt_value(x[i], key, O.device_r(RK, 9 + i, rbytes) % key.n)
    finally:
        ctx.close()
