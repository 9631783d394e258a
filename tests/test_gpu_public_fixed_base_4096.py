"""GPU parity of the 2049..4096-bit public fixed-base sampler (kernels_pfb4.hpp: k_pfb4, PAI_OPT_PUBLIC_FB = 2) against
the oracle's restatement of the reference's ciphertext under the sampler's r (oracle/paillier_oracle.py pfb_*), at the two
edges of its key range (tests/golden/pfb4_keys.json: n of 4096 bits with its top limb all ones, n of 2049 bits); the same
r^n on pai_obfuscate; the break-even; and the default option value, which leaves such a context on k_pe4_*."""
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

RK = bytes(range(60, 92))
WANT = {}   # (n, window, global index, x) -> the oracle's (ciphertext, exponent)


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(os.path.dirname(__file__), "golden", "pfb4_keys.json")) as f:
        ks = json.load(f)["keys"]
    return {name: (O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16)), [int(b, 16) for b in k["bases"]])
            for name, k in ks.items()}


# W = 16 on one key only: its tables are about 36 GB
@pytest.fixture(scope="module", params=[("4096_top_limb_full", 12), ("4096_top_limb_full", 16), ("2049", 12)],
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
@pytest.mark.parametrize("count", [1, 33, 300])
def test_encrypt_matches_oracle(sampler, count, index_base):
    N = _native()
    ctx, key, bases, window = sampler
    assert ctx.pfb_ready
    gb, K, W, K0 = ctx.public_fixed_base_info()
    assert gb == bases and W == window and (K0, (K - K0) // O.PFB_SHORT) == O.pfb_layout(key.n.bit_length(), window)
    x = (np.random.default_rng(7).standard_normal(300) * 100).astype(np.float32)[:count]   # one prefix for every count
    x[0] = 0.0
    x[-1] = -3.25
    ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=index_base)
    assert np.all(st == 0)
    got = N.words_to_ints(ct)
    # one group, one element past a 32-group block, several blocks with a partial tail: elements 0..33 (index_base + i
    # crosses 2^32 at i = 3), the block seams, the last element and every 37th between. The oracle's 8192-bit
    # exponentiation (half a second per element at 4096 bits) is the test's time: the counts share what they have in common.
    for i in sorted(i for i in set(range(34)) | {63, 64, 65, count - 1} | set(range(34, count, 37)) if i < count):
        ref = (key.n, window, index_base + i, float(x[i]))
        if ref not in WANT:
            WANT[ref] = O.pfb_encrypt_value(x[i], key, bases, RK, index_base + i, window)
        assert (got[i], int(ex[i])) == WANT[ref], f"element {i}"


def test_obfuscate_draws_the_same_r(keys):
    """pai_obfuscate multiplies by the r^n that pai_encrypt of zeros gives at the same key and indices."""
    N = _native()
    key, bases = keys["4096_top_limb_full"]
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
    """Opted in and unprepared, a context builds its tables only past the break-even of profiles/pfb4_rate.json, measured
    at 4096 bits: the first build's time as a line through the two windows, over the time an element saves, k_pe4_*'s
    scaled by the bits of n and k_pfb4's by its positions (pfb_threshold); a call below it stays on k_pe4_*."""
    monkeypatch.delenv("FLEXPAI_PFB_MIN_ELEMS", raising=False)
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "pfb4_rate.json")) as f:
        m = json.load(f)
    w12, w16 = m["k_pfb4_w12"], m["k_pfb4_w16"]
    per_row = (w16["build_s"][0] - w12["build_s"][0]) / (w16["rows"] - w12["rows"])
    key, _ = keys["2049"]
    ctx = _native().Context(key.n, 0)
    try:
        ctx.set_public_fixed_base(2)
        K0, KS = O.pfb_layout(2049, 16)
        K = K0 + O.PFB_SHORT * KS
        build_s = w12["build_s"][0] + ((K << 16) - w12["rows"]) * per_row
        saved_s = 2049 / m["nb"] / m["k_pe4"]["encrypts_per_s"] - K / (w16["rows"] >> 16) / w16["encrypts_per_s"]
        want = int(build_s / saved_s) + 1
        assert abs(ctx.public_fixed_base_policy()[1] - want) <= 1 and 2 * 65 < want
        ctx.encrypt(np.ones(65, dtype=np.float32), obf_mode=_native().PAI_OBF_RNG, rng_key=RK)
        assert not ctx.pfb_ready and ctx.public_fixed_base_policy()[0] == 65
    finally:
        ctx.close()


def test_default_option_keeps_the_per_element_chain(keys):
    """PAI_OPT_PUBLIC_FB = 1 (the default): no tables at these sizes, and the ChaCha20-r ciphertexts of k_pe4_* (on the
    short key: the oracle's 65 exponentiations take 25 s at 4096 bits)."""
    N = _native()
    key, bases = keys["2049"]
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
