"""The obfuscator pool through the C ABI (include/flexpai.h "Obfuscator pool"; csrc/kernels_pool.hpp: k_pool_split,
k_pool_enc, k_pool_join): r^n drawn ahead of time into the context's ring, and pooled encryption / re-randomisation that
spends one entry per element, in order, exactly once.

  1. goldens          pool filled with the r of the reference's records, pooled encryption = their c and e, bit for bit
  2. route's E0       fill(PAI_OBF_RNG) then pooled encryption of zeros = the ordinary device-RNG encryption of zeros
  3. the identity     pai_pool_put of edge and random rho, every key size and seam, F32 / F64 / I64, both exponent modes:
                      c0 rho mod n^2 in Python integers, exponents and statuses of the PAI_OBF_NONE call
  4. fused = composed PAI_OPT_POOL_FUSED 0 and 1: identical words
  5. ring             wrap-around take, FIFO pairing, pool_info at every step
  6. refusals         each leaves the state untouched
  7. obfuscate        c rho mod n^2 out of place, in place, sliced; the _dev entry points on a side stream
  8. threads          two threads on one context: every row exactly once
  9. package          prepare_obfuscators and its consumers

Every exponentiation count is at most 64, so even the 4096-bit fills stay in the row kernels."""
import threading

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
# name -> (bits of n, bits of the two primes, first seed tried, lanes per group): tests/test_gpu_ops_sizes.py's table
GENERATED = {"K1035": (1035, 518, 517, 1, 2), "K1036": (1036, 518, 518, 1, 4), "K2071": (2071, 1036, 1035, 1, 4),
             "K2072": (2072, 1036, 1036, 1, 8), "K3072": (3072, 1536, 1536, 2, 8)}
LANES = {"K512": 2, "K4096": 8, **{k: v[4] for k, v in GENERATED.items()}}
ALL_KEYS = ["K512", "K1035", "K1036", "K2071", "K2072", "K3072", "K4096"]
GOLDEN_LANES = {1024: 2, 2048: 4, 4096: 8}


def _native():
    from flex.crypto.paillier import _native
    return _native


def _golden_key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _make_key(name, golden):
    if name == "K512":
        k = next(e for e in golden["keygen"] if e["nb"] == 512 and e["seed"] == 99)
        return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    if name == "K4096":
        return _golden_key(golden, 4096)
    nb, pb, qb, seed, _ = GENERATED[name]
    while True:                                      # step the seed until n has exactly nb bits
        p, q = O.getprimeover(pb, seed=seed), O.getprimeover(qb, seed=seed + 1000)
        if p != q and (p * q).bit_length() == nb:
            return O.Key(p * q, p, q)
        seed += 1


@pytest.fixture(scope="module")
def gkeys(golden):
    return {nb: _golden_key(golden, nb) for nb in (1024, 2048, 4096)}


def _public(key):
    return _native().Context(key.n, 0)


def _rand_below(rng, bound):
    nbytes = (bound.bit_length() + 7) // 8 + 8
    return int.from_bytes(rng.bytes(nbytes), "little") % bound


def _rhos(rng, key, count):
    """The edge set, then random rows, cycling."""
    n, n2 = key.n, key.nsquare
    edges = [1, 2, n - 1, n, n + 1, n2 - n, n2 - 1]
    return [edges[i % 14] if i % 14 < 7 else _rand_below(rng, n2) for i in range(count)]


def _refused(fn, *a, **kw):
    N = _native()
    with pytest.raises(N.NativeError, match="flexpai error -1"):
        fn(*a, **kw)


# ---------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("nb", [1024, 2048, 4096])
def test_goldens_through_the_pool(golden, gkeys, nb):
    N = _native()
    ctx = _public(gkeys[nb])
    recs = golden["encrypt"][str(nb)][:24 if nb == 4096 else 64]
    count = len(recs)
    x = np.array([r["bits"] for r in recs], dtype=np.uint32).view(np.float32)
    ctx.pool_reserve(64)
    ctx.pool_fill(count, N.PAI_OBF_GIVEN, r=[int(r["r"], 16) for r in recs])
    assert ctx.pool_info() == (64, count, 0)
    ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_POOL)
    got = N.words_to_ints(ct)
    for i, rec in enumerate(recs):
        assert st[i] == 0
        assert (hex(got[i]), int(ex[i])) == (rec["c"], rec["e"]), f"element {i}"
    assert ctx.pool_info() == (64, 0, count)


# ---------------------------------------------------------------- 2. entries are the route's E0
@pytest.mark.parametrize("holder", [False, True])
def test_fill_is_the_encryption_of_zero(gkeys, holder):
    N = _native()
    key = gkeys[2048]
    rk, base = bytes(range(7, 39)), 2 ** 34 + 5
    zeros = np.zeros(40, dtype=np.int64)
    a = N.Context(key.n, 0, key.p, key.q) if holder else _public(key)
    b = N.Context(key.n, 0, key.p, key.q) if holder else _public(key)
    if holder:
        for c in (a, b):
            c.set_fb_window(8)
    a.pool_reserve(40)
    a.pool_fill(40, N.PAI_OBF_RNG, rng_key=rk, index_base=base)
    got, ea, sa = a.encrypt(zeros, obf_mode=N.PAI_OBF_POOL)
    want, eb, sb = b.encrypt(zeros, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=base)
    assert np.array_equal(got, want) and np.array_equal(ea, eb) and np.array_equal(sa, sb)
    if holder:
        assert a.fb_ready and b.fb_ready and a.fixed_base_policy() == b.fixed_base_policy()
    else:
        assert a.public_fixed_base_policy() == b.public_fixed_base_policy()
    assert len(set(N.words_to_ints(got))) == 40


# ---------------------------------------------------------------- 3. the identity, via pai_pool_put
F_VALUES = [0.0, -0.0, 1.0, -1.0, 1.7, -1.7, 1e-45, -1e-45, 3.4e38, -3.4e38]
I_VALUES = [0, 1, -1, 2, -2, 2 ** 63 - 1, -(2 ** 63 - 1), 2 ** 28, -(2 ** 56)]
FIXED_EXP = {np.float32: -17, np.float64: -17, np.int64: -2}   # every listed value stays inside int64: 3.4e38 16^-17 < 2^61


def _plain(rng, dt, fixed, count):
    """The listed values cycling with random ones, and (floats) three bad elements at fixed places: NaN, +inf and a value
    out of the fixed exponent's range (float64 1e300; float32 has none below inf at an exponent that keeps 3.4e38, so
    -inf stands in). Under PAI_EXP_AUTO every finite float encodes, so the third is then an ordinary element."""
    if dt == np.int64:
        vals = [I_VALUES[i % 12] if i % 12 < len(I_VALUES) else int(rng.integers(-2 ** 62, 2 ** 62)) for i in range(count)]
        return np.array(vals, dtype=np.int64), []
    lo, hi = (20, 37) if fixed else (-6, 7)            # at the fixed exponent only large values have a non-zero mantissa
    x = np.array([F_VALUES[i % 13] if i % 13 < len(F_VALUES) else
                  float(np.clip(rng.standard_normal(), -3, 3) * 10.0 ** rng.integers(lo, hi)) for i in range(count)],
                 dtype=np.float64)
    if dt == np.float64:
        x[11], x[24] = 2.0 ** 63 - 1024, -(2.0 ** 63 - 1024)
    bad = [5, 17, 30]
    x[5], x[17] = np.nan, np.inf
    x[30] = 1e300 if dt == np.float64 else -np.inf
    with np.errstate(over="ignore"):
        return x.astype(dt), bad


def _identity_case(ctx, key, lanes, dt, fixed, seed):
    """One pooled call against Python integers; returns its words for the fused / composed comparison."""
    N = _native()
    rng = np.random.default_rng(seed)
    count = 256 // lanes + 3                           # a tail block, odd
    x, bad = _plain(rng, dt, fixed, count)
    mode, fexp = (N.PAI_EXP_FIXED, FIXED_EXP[dt]) if fixed else (N.PAI_EXP_AUTO, 0)
    c0w, e0, s0 = ctx.encrypt(x, exp_mode=mode, fixed_exp=fexp, obf_mode=N.PAI_OBF_NONE)
    rhos = _rhos(rng, key, count)
    ctx.pool_reserve(count)
    ctx.pool_put(rhos)
    taken = ctx.pool_info()[2]
    ct, ex, st = ctx.encrypt(x, exp_mode=mode, fixed_exp=fexp, obf_mode=N.PAI_OBF_POOL)
    assert ctx.pool_info() == (count, 0, taken + count)   # the bad elements consumed their entries too
    assert np.array_equal(st, s0), "statuses are those of the PAI_OBF_NONE call"
    left_out = [i for i in range(count) if s0[i] != N.EL_OK]
    assert set(left_out) <= set(bad), f"only the bad elements may be left out, got {left_out}"
    assert all(s0[i] != N.EL_OK for i in bad[:2]) and (not fixed or not bad or s0[bad[2]] != N.EL_OK)
    keep = [i for i in range(count) if i not in left_out]
    assert np.array_equal(ex[keep], e0[keep])
    got, c0 = N.words_to_ints(ct), N.words_to_ints(c0w)
    wrong = [i for i in keep if got[i] != c0[i] * rhos[i] % key.nsquare]
    assert not wrong, f"{len(wrong)} of {len(keep)} differ from c0 rho mod n^2, first at {wrong[:8]}"
    ones = [i for i in keep if rhos[i] == 1]
    assert ones and all(got[i] == c0[i] for i in ones)
    return ct


@pytest.mark.parametrize("name", ALL_KEYS)
def test_identity_at_every_key_size(golden, name):
    key = _make_key(name, golden)
    ctx = _public(key)
    assert ctx.pool_fused
    seed = 100
    for dt in (np.float32, np.float64, np.int64):
        for fixed in (False, True):
            _identity_case(ctx, key, LANES[name], dt, fixed, seed)
            seed += 1


# ---------------------------------------------------------------- 4. fused against composed
@pytest.mark.parametrize("nb", [1024, 2048, 4096])
def test_fused_and_composed_agree(gkeys, nb):
    key = gkeys[nb]
    ctx = _public(key)
    seed = 200
    for dt in (np.float32, np.float64, np.int64):
        for fixed in (False, True):
            ctx.set_pool_fused(True)
            fused = _identity_case(ctx, key, GOLDEN_LANES[nb], dt, fixed, seed)
            ctx.set_pool_fused(False)
            assert not ctx.pool_fused
            composed = _identity_case(ctx, key, GOLDEN_LANES[nb], dt, fixed, seed)
            assert np.array_equal(fused, composed)
            seed += 1


# ---------------------------------------------------------------- 5. ring
def test_ring_wraps_in_fifo_order(gkeys):
    N = _native()
    key = gkeys[2048]
    ctx = _public(key)
    rng = np.random.default_rng(5)
    rhos = _rhos(rng, key, 124)
    x = rng.standard_normal(124).astype(np.float64)
    c0 = N.words_to_ints(ctx.encrypt(x, obf_mode=N.PAI_OBF_NONE)[0])
    ctx.pool_reserve(96)
    assert ctx.pool_info() == (96, 0, 0)
    ctx.pool_put(rhos[:64])
    assert ctx.pool_info() == (96, 64, 0)
    first = N.words_to_ints(ctx.encrypt(x[:40], obf_mode=N.PAI_OBF_POOL)[0])
    assert ctx.pool_info() == (96, 24, 40)
    ctx.pool_put(rhos[64:])                              # 60 more: rows 64 .. 95, then 0 .. 27
    assert ctx.pool_info() == (96, 84, 40)
    second = N.words_to_ints(ctx.encrypt(x[40:], obf_mode=N.PAI_OBF_POOL)[0])   # one call over the seam
    assert ctx.pool_info() == (96, 0, 124)
    got = first + second
    wrong = [i for i in range(124) if got[i] != c0[i] * rhos[i] % key.nsquare]
    assert not wrong, f"outputs that do not pair with their rho in FIFO order: {wrong[:8]}"


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_state_untouched(gkeys):
    N = _native()
    key = gkeys[1024]
    ctx = _public(key)
    x = np.arange(8, dtype=np.int64)
    _refused(ctx.encrypt, x, obf_mode=N.PAI_OBF_POOL)                   # no pool
    _refused(ctx.obfuscate, ctx.encrypt(x, obf_mode=N.PAI_OBF_NONE)[0], obf_mode=N.PAI_OBF_POOL)
    _refused(ctx.pool_put, [1, 2])
    assert ctx.pool_info() == (0, 0, 0)
    ctx.pool_reserve(8)
    ctx.pool_put([3, 5, 7, 11, 13])
    state = (8, 5, 0)
    with pytest.raises(N.NativeError, match=r"takes 6 obfuscators, the pool holds 5"):
        ctx.encrypt(x[:6], obf_mode=N.PAI_OBF_POOL)
    assert ctx.pool_info() == state
    _refused(ctx.obfuscate, ctx.encrypt(x[:6], obf_mode=N.PAI_OBF_NONE)[0], obf_mode=N.PAI_OBF_POOL)
    assert ctx.pool_info() == state
    _refused(ctx.pool_put, [17, 19, 23, 29])                            # 4 > 3 free
    _refused(ctx.pool_fill, 4, N.PAI_OBF_RNG, rng_key=bytes(32))
    _refused(ctx.pool_fill, 1, N.PAI_OBF_NONE)
    _refused(ctx.pool_fill, 1, N.PAI_OBF_POOL)
    assert ctx.pool_info() == state
    lay = (32, 24, 4, 4)
    _refused(ctx.encrypt_packed, np.ones(8), lay, obf_mode=N.PAI_OBF_POOL)
    assert ctx.pool_info() == state
    # what is there still serves: the five entries in order
    ct = N.words_to_ints(ctx.encrypt(np.zeros(5, dtype=np.int64), obf_mode=N.PAI_OBF_POOL)[0])
    assert ct == [3, 5, 7, 11, 13] and ctx.pool_info() == (8, 0, 5)
    ctx.pool_put([2])
    ctx.pool_reserve(0)                                                 # frees the ring
    assert ctx.pool_info() == (0, 0, 5)
    _refused(ctx.encrypt, x[:1], obf_mode=N.PAI_OBF_POOL)
    ctx.pool_reserve(4)
    ctx.pool_put([2, 3])
    ctx.set_private(key.p, key.q)                                       # re-keying drops the pool
    assert ctx.pool_info() == (0, 0, 5)
    _refused(ctx.encrypt, x[:1], obf_mode=N.PAI_OBF_POOL)


# ---------------------------------------------------------------- 7. obfuscate from the pool
def _golden_cts(golden, ctx, nb, count):
    N = _native()
    recs = golden["encrypt"][str(nb)]
    return N.ints_to_words([int(recs[i % len(recs)]["c"], 16) for i in range(count)], ctx.ct_words)


def test_obfuscate_from_the_pool(golden, gkeys):
    N = _native()
    key = gkeys[2048]
    ctx = _public(key)
    rng = np.random.default_rng(7)
    ct = _golden_cts(golden, ctx, 2048, 131)
    cs = N.words_to_ints(ct)
    ctx.pool_reserve(131)
    ctx.set_obf_chunk(64)                                 # the in-place device call below walks 64, 64 and 3
    for in_place in (False, True):
        rhos = _rhos(rng, key, 131)
        ctx.pool_put(rhos)
        buf = ct.copy()
        out = ctx.obfuscate(buf, obf_mode=N.PAI_OBF_POOL, out=buf if in_place else None)
        assert ctx.pool_info()[1] == 0
        got = N.words_to_ints(out)
        wrong = [i for i in range(131) if got[i] != cs[i] * rhos[i] % key.nsquare]
        assert not wrong, f"in_place={in_place}: {wrong[:8]}"
        if not in_place:
            assert np.array_equal(buf, ct)


@pytest.mark.parametrize("in_place", [False, True])
def test_dev_entry_points_on_a_side_stream(golden, gkeys, in_place):
    """pai_pool_put_dev, pai_obfuscate_dev and pai_encrypt_dev on torch buffers and a stream of their own."""
    torch = pytest.importorskip("torch")
    N = _native()
    key = gkeys[2048]
    ctx = _public(key)
    lib = ctx.lib
    rng = np.random.default_rng(11)
    count = 131
    ct = _golden_cts(golden, ctx, 2048, count)
    cs = N.words_to_ints(ct)
    rhos = _rhos(rng, key, 2 * count)
    dev = torch.device("cuda", 0)
    ctx.pool_reserve(2 * count)
    ctx.set_obf_chunk(64)
    d_rho = torch.from_numpy(N.ints_to_words(rhos, ctx.ct_words).view(np.int32)).to(dev)
    d_ct = torch.from_numpy(ct.view(np.int32)).to(dev)
    d_out = d_ct if in_place else torch.empty_like(d_ct)
    x = rng.standard_normal(count)
    d_x = torch.from_numpy(x).to(dev)
    d_enc = torch.empty_like(d_ct)
    d_exp = torch.empty(count, dtype=torch.int32, device=dev)
    d_st = torch.empty(count, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    rc = lib.pai_pool_put_dev(ctx.handle, d_rho.data_ptr(), 2 * count, stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    rc = lib.pai_obfuscate_dev(ctx.handle, d_ct.data_ptr(), count, N.PAI_OBF_POOL, None, 0, 0, None, 0, d_out.data_ptr(),
                               stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    rc = lib.pai_encrypt_dev(ctx.handle, N.PAI_F64, d_x.data_ptr(), count, N.PAI_EXP_AUTO, 0, N.PAI_OBF_POOL, None, 0, 0,
                             None, 0, d_enc.data_ptr(), d_exp.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    stream.synchronize()
    assert ctx.pool_info() == (2 * count, 0, 2 * count)
    got = N.words_to_ints(d_out.cpu().numpy().view(np.uint32))
    wrong = [i for i in range(count) if got[i] != cs[i] * rhos[i] % key.nsquare]
    assert not wrong, f"pai_obfuscate_dev: {wrong[:8]}"
    c0w, e0, s0 = ctx.encrypt(x, obf_mode=N.PAI_OBF_NONE)
    c0 = N.words_to_ints(c0w)
    enc = N.words_to_ints(d_enc.cpu().numpy().view(np.uint32))
    wrong = [i for i in range(count) if enc[i] != c0[i] * rhos[count + i] % key.nsquare]
    assert not wrong, f"pai_encrypt_dev: {wrong[:8]}"
    assert np.array_equal(d_exp.cpu().numpy(), e0) and np.array_equal(d_st.cpu().numpy(), s0)


# ---------------------------------------------------------------- 8. threads
def test_two_threads_take_every_row_exactly_once(gkeys):
    N = _native()
    key = gkeys[1024]
    ctx = _public(key)
    rhos = [_rand_below(np.random.default_rng(13 + i), key.nsquare) for i in range(96)]
    assert len(set(rhos)) == 96
    ctx.pool_reserve(96)
    ctx.pool_put(rhos)
    zeros = np.zeros(6, dtype=np.int64)
    outs, errs = [[], []], []

    def work(t):
        try:
            for _ in range(8):
                outs[t].append(N.words_to_ints(ctx.encrypt(zeros, obf_mode=N.PAI_OBF_POOL)[0]))
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    calls = outs[0] + outs[1]
    got = [v for call in calls for v in call]
    assert sorted(got) == sorted(rhos), "the 96 outputs are the 96 rows, each exactly once"
    starts = sorted(rhos.index(call[0]) for call in calls)
    assert starts == list(range(0, 96, 6)) and all(call == rhos[rhos.index(call[0]):][:6] for call in calls)
    assert ctx.pool_info() == (96, 0, 96)


# ---------------------------------------------------------------- 9. package
def test_package_consumers(gkeys):
    from flex.crypto.paillier import obfuscator_pool
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    key = gkeys[2048]
    pk = PaillierPublicKey(key.n)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))
    rng = np.random.default_rng(9)
    x = rng.standard_normal(60).astype(np.float32)          # float32: exact round trip
    src = enc.encrypt_to_buffer(rng.standard_normal(30).astype(np.float32))   # before any pool: the ordinary route
    want30 = dec.decrypt(src) * 2
    assert enc.obfuscators_ready() == 0
    try:
        assert enc.prepare_obfuscators(100) == 100 and enc.obfuscators_ready() == 100
        first = enc.encrypt(x)
        assert enc.obfuscators_ready() == 40 and np.array_equal(dec.decrypt(first), x.astype(np.float64))
        second = enc.encrypt(x)                              # 60 > 40: the ordinary route, pool untouched
        assert enc.obfuscators_ready() == 40 and np.array_equal(dec.decrypt(second), x.astype(np.float64))
        assert all(a.ciphertext(False) != b.ciphertext(False) for a, b in zip(first, second))
        one = enc.encrypt(0.75)
        assert enc.obfuscators_ready() == 39 and dec.decrypt(one) == 0.75
        total = src + src
        assert not total.obfuscated.any()
        before = total.words.copy()
        total.apply_obfuscation()
        assert enc.obfuscators_ready() == 9 and total.obfuscated.all()
        assert not np.array_equal(total.words, before) and np.array_equal(dec.decrypt(total), want30)
    finally:
        obfuscator_pool.drop(pk)
    assert enc.obfuscators_ready() == 0
