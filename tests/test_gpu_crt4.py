"""GPU parity of the split-pair CRT encryption of a 2049..4096-bit key holder above the row kernels' range
(kernels_crt4.hpp: k_crt4_pre + k_crt4_a, k_crt4_b, k_crt_fin<8>) against the reference golden vectors (explicit r), the
CPU oracle and the kernel those calls ran on before (k_encrypt<8>, PAI_OPT_CRT_ENCRYPT = 0 in the same library):
bit-identical ciphertexts, exponents, statuses.

The oracle's r^n mod n^2 at 4096 bits takes most of a second on the host, so the cases that compare the same elements
share one set of oracle values (module fixtures), and the array-wide comparisons are against k_encrypt<8>."""
import collections

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(32))
RBYTES = ((4096 + 64 + 31) // 32) * 4        # bytes of the ChaCha20 stream k_encrypt and k_crt4_pre draw
CHUNK = 1 << 18                              # launch_crt4's chunk (flexpai.hip CRT4_CHUNK)


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def key4096(golden):
    k = golden["keys"]["4096"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _holder(key, crt=True, rows_max=0, crt4_min=0):
    """A key holder's context of the product library with the fixed bases off and neither the rows nor the floor in
    the way; crt=False: the same calls on k_encrypt<8>."""
    N = _native()
    c = N.Context(key.n, 0, key.p, key.q)
    c.set_fixed_base(False)
    if rows_max is not None:
        c.set_rows_max(rows_max)
    if crt4_min is not None:
        c.set_crt4_min(crt4_min)
    if not crt:
        c.set_crt(False)
    return c


@pytest.fixture(scope="module")
def ab(key4096):
    return _holder(key4096), _holder(key4096, crt=False)


def _stages(ctx, *args, **kw):
    ctx.set_stage_timing(True)
    try:
        ctx.encrypt(*args, **kw)
        return len(ctx.stage_times())
    finally:
        ctx.set_stage_timing(False)


def _same(ra, rb):
    return all(np.array_equal(u, v) for u, v in zip(ra, rb))


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    x[::7] = 0.0
    x[1::9] = -x[1::9]
    return x


# ---------------------------------------------------------------- 1. the path is taken
def test_crt4_path_is_taken(monkeypatch, ab, key4096):
    N = _native()
    a, b = ab
    assert a.pair_paths & 8, "the key holder's encryption above the rows runs the split-pair CRT"
    assert not a.pair_paths & 4, "a key holder's bit 2 stays 0"
    assert a.crt4_min == 0 and N.Context(key4096.n, 0, key4096.p, key4096.q).crt4_min == 128
    x = _mixed(33, 1)
    kw = dict(obf_mode=N.PAI_OBF_GIVEN, r=[7 + i for i in range(33)])
    assert _stages(a, x, **kw) == 3, "stage A, stage B, finish"
    assert _stages(b, x, **kw) == 1, "k_encrypt<8>"
    # the default floor: one block of lane pairs stays on k_encrypt<8>
    d = _holder(key4096, crt4_min=None)
    assert d.crt4_min == 128
    assert _stages(d, _mixed(128, 2), obf_mode=N.PAI_OBF_GIVEN, r_scalar=12345) == 1
    assert _stages(d, _mixed(129, 2), obf_mode=N.PAI_OBF_GIVEN, r_scalar=12345) == 3
    # library defaults: the rows take calls of up to 4096 elements (k_crt_w, k_crt_fin)
    e = _holder(key4096, rows_max=None, crt4_min=None)
    assert _stages(e, _mixed(4097, 3), obf_mode=N.PAI_OBF_GIVEN, r_scalar=12345) == 3
    assert _stages(e, _mixed(4096, 3), obf_mode=N.PAI_OBF_GIVEN, r_scalar=12345) == 2
    # the test build's contexts (the cross-checks' references) stay on the kernels they had
    xl = N.load_library(N.XCHECK_LIB_PATH)
    assert not N.Context(key4096.n, 0, key4096.p, key4096.q, lib=xl).pair_paths & 8
    monkeypatch.setenv("FLEXPAI_PAIR", "0")
    assert not N.Context(key4096.n, 0, key4096.p, key4096.q, lib=xl).pair_paths & 8
    monkeypatch.delenv("FLEXPAI_PAIR")
    pub = N.Context(key4096.n, 0)
    assert not pub.pair_paths & 8 and pub.pair_paths & 4, "a public-key-only context: pair groups, no CRT"


# ---------------------------------------------------------------- 2. goldens
def test_crt4_given_r_matches_reference_goldens(golden, ab):
    N = _native()
    a, _ = ab
    recs = golden["encrypt"]["4096"]
    assert len(recs) == 24
    x = np.array([r["bits"] for r in recs], dtype=np.uint32).view(np.float32)
    ct, ex, st = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=[int(r["r"], 16) for r in recs])
    got = N.words_to_ints(ct)
    for i, rec in enumerate(recs):
        assert st[i] == 0
        assert (hex(got[i]), int(ex[i])) == (rec["c"], rec["e"]), f"element {i}"


# ---------------------------------------------------------------- 3. ragged counts
X300 = _mixed(300, 300)          # every count encrypts a prefix of one array: the oracle values of its head are shared
X300[:4] = np.array([3.25e-7, -41.5, 0.0, 6.0e20], dtype=np.float32)
F64 = X300[:4].astype(np.float64) * (1.0 + 2.0 ** -40)
I64 = np.array([0, -1, 2 ** 40 + 1, -(2 ** 52)], dtype=np.int64)


@pytest.fixture(scope="module")
def head_oracle(key4096):
    def ref(x):
        return [O.encrypt_value(x[i], key4096, O.device_r(KEY32, 77 + i, RBYTES)) for i in range(4)]
    return {"f32": ref(X300), "f64": ref(F64), "i64": ref(I64)}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300])
def test_crt4_ragged_counts_match_k_encrypt_and_oracle(ab, head_oracle, n):
    """Either side of a wave's 32 lane pairs, of a stage-B block's 128 pairs and of a stage-A block's 256 lanes."""
    N = _native()
    a, b = ab
    x = X300[:n]
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=77)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0][: min(n, 4)])
    for i in range(min(n, 4)):
        assert (got[i], int(ra[1][i])) == head_oracle["f32"][i], f"element {i}"


# ---------------------------------------------------------------- 4. dtypes and exponent modes
@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_crt4_other_dtypes(ab, head_oracle, kind):
    N = _native()
    a, b = ab
    rng = np.random.default_rng(64)
    if kind == "f64":
        x = rng.standard_normal(33) * 10.0 ** rng.integers(-30, 30, 33)
        x[:4] = F64
    else:
        x = rng.integers(-2 ** 53, 2 ** 53, 33, dtype=np.int64)
        x[:4] = I64
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=77)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0][:4])
    for i in range(4):
        assert (got[i], int(ra[1][i])) == head_oracle[kind][i], f"element {i}"


@pytest.mark.parametrize("fexp", [-8, 3, 40])
def test_crt4_fixed_exponent(ab, fexp):
    N = _native()
    a, b = ab
    x = _mixed(33, 44)
    kw = dict(exp_mode=N.PAI_EXP_FIXED, fixed_exp=fexp, obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=5)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)


# ---------------------------------------------------------------- 5. edge obfuscators
def test_crt4_edge_obfuscators(ab, key4096):
    """r = 0, 1, 2, n - 1, n, n + 1, multiples of p and q (non-units), p^2, n^2 - 1, all-ones words (r >= n^2)."""
    N = _native()
    a, b = ab
    k = key4096
    rs = [0, 1, 2, k.n - 1, k.n, k.n + 1, 5 * k.p, 3 * k.q, k.p * k.p, k.nsquare - 1, (1 << (32 * a.ct_words)) - 1]
    x = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e30, 3.5, -2.25, 7.0, 0.5, -0.125], dtype=np.float32)
    ra = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    rb = b.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    for i, r in enumerate(rs):
        assert (got[i], int(ra[1][i])) == O.encrypt_value(x[i], k, r), f"r #{i}"


def _encrypt_words(ctx, x, r_words_arr):
    """pai_encrypt with r as [N, w] uint32 words (w may be below ct_words)."""
    N = _native()
    n = x.size
    ct = np.empty((n, ctx.ct_words), dtype=np.uint32)
    ex = np.empty(n, dtype=np.int32)
    st = np.empty(n, dtype=np.int32)
    r = np.ascontiguousarray(r_words_arr, dtype=np.uint32)
    rc = ctx.lib.pai_encrypt(ctx.handle, N.PAI_F32, x.ctypes.data, n, N.PAI_EXP_AUTO, 0, N.PAI_OBF_GIVEN, r.ctypes.data,
                             r.shape[1] * 4, r.shape[1] * 4, None, 0, ct.ctypes.data, ex.ctypes.data, st.ctypes.data)
    assert rc == 0, ctx.lib.pai_last_error().decode()
    return ct, ex, st


def test_crt4_short_r(ab, key4096):
    """r_words = 1: one chunk of the reduction, most of its digits past the words."""
    N = _native()
    a, b = ab
    x = np.array([1.5, -2.0, 0.0], dtype=np.float32)
    r = np.array([[0xFFFFFFFF], [1], [0x12345678]], dtype=np.uint32)
    ra, rb = _encrypt_words(a, x, r), _encrypt_words(b, x, r)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    assert (got[0], int(ra[1][0])) == O.encrypt_value(x[0], key4096, 0xFFFFFFFF)


# ---------------------------------------------------------------- 6. one r for all elements
def test_crt4_one_r_for_all_elements(ab, key4096):
    """r_stride 0: every element reads the same words."""
    N = _native()
    a, b = ab
    r = int.from_bytes(np.random.default_rng(9).bytes(1024), "little") % key4096.nsquare
    x = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e30, 2.5, -1234.5, 1e-3], dtype=np.float32)
    ra = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r_scalar=r)
    rb = b.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r_scalar=r)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    for i in range(x.size):
        assert (got[i], int(ra[1][i])) == O.encrypt_value(x[i], key4096, r), f"element {i}"


# ---------------------------------------------------------------- 7. other keys
_SMALL = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97)


def _probable(n, rng):
    if any(n % sp == 0 for sp in _SMALL):
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        x = pow(int(rng.integers(2, 1 << 62)) % (n - 3) + 2, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _prime(bits, rng):
    """A random prime of exactly `bits` bits (Miller-Rabin, 24 random bases)."""
    while True:
        c = int.from_bytes(rng.bytes((bits + 7) // 8), "little") % (1 << bits) | (1 << (bits - 1)) | 1
        if _probable(c, rng):
            return c


def _prime_below(v, rng):
    v -= 1 if v % 2 == 0 else 2
    while not _probable(v, rng):
        v -= 2
    return v


def _other_key(kind):
    rng = np.random.default_rng(3072)
    if kind == "3072":
        p, q = sorted((_prime(1536, rng), _prime(1536, rng)))
    else:                                    # the two largest primes below 2^2048: the R >= 2^24 p_h bound at its top
        q = _prime_below(1 << 2048, rng)
        p = _prime_below(q, rng)
    return O.Key(p * q, p, q)


@pytest.mark.parametrize("kind", ["3072", "largest-halves"])
def test_crt4_other_keys(kind):
    N = _native()
    key = _other_key(kind)
    a, b = _holder(key), _holder(key, crt=False)
    assert a.pair_paths & 8
    rng = np.random.default_rng(key.n.bit_length())
    rs = [int.from_bytes(rng.bytes(1024), "little") % key.nsquare for _ in range(9)]
    x = _mixed(9, 5)
    assert _stages(a, x, obf_mode=N.PAI_OBF_GIVEN, r=rs) == 3
    ra = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    rb = b.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    for i in (0, 4, 8):
        assert (got[i], int(ra[1][i])) == O.encrypt_value(x[i], key, rs[i]), f"element {i}"
    val, _, _, _ = a.decrypt(ra[0], ra[1])
    assert np.array_equal(val, x.astype(np.float64))


# ---------------------------------------------------------------- 8. the grid-stride loops
def test_crt4_grid_stride_loop(ab, key4096):
    """40 003 elements: more than a grid holds at once -- stage A (one wave per SIMD, one 256-lane block per CU, the two
    halves on blockIdx.y) 128 blocks x 256 = 32 768 elements per half, stage B 128 blocks x 128 lane pairs = 16 384 -- so
    the blocks of both walk their loops more than once, with a ragged tail."""
    N = _native()
    a, b = ab
    n = 40003
    x = (np.random.default_rng(6).standard_normal(n) * 1000).astype(np.float32)
    rk = bytes(range(3, 35))
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=2 ** 34)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)
    idx = [0, 20001, 40002]
    got = N.words_to_ints(ra[0][idx])
    for j, i in enumerate(idx):
        assert (got[j], int(ra[1][i])) == O.encrypt_value(x[i], key4096, O.device_r(rk, 2 ** 34 + i, RBYTES))
    val, _, _, _ = a.decrypt(ra[0], ra[1])
    assert np.array_equal(val, x.astype(np.float64))


# ---------------------------------------------------------------- 9. launch_crt4's chunk boundary
def _encrypt_dev(ctx, x, rk, index_base):
    """pai_encrypt_dev on device buffers (the host entry point cuts a call into chunks of its own, below CHUNK)."""
    import torch
    N = _native()
    dev = torch.device("cuda", 0)
    n = x.size
    dx = torch.from_numpy(x).to(dev)
    ct = torch.empty((n, ctx.ct_words), dtype=torch.int32, device=dev)
    ex = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    rc = ctx.lib.pai_encrypt_dev(ctx.handle, N.PAI_F32, dx.data_ptr(), n, 0, 0, N.PAI_OBF_RNG, None, 0, 0, rk, index_base,
                                 ct.data_ptr(), ex.data_ptr(), st.data_ptr(), None)
    assert rc == 0, ctx.lib.pai_last_error().decode()
    torch.cuda.synchronize()
    return ct, ex, st


def test_crt4_chunk_boundary(ab, key4096):
    """2^18 + 3 elements in one device call: launch_crt4 runs two chunks, the second with r's index base and every
    pointer advanced by 2^18. The 5 elements around the boundary equal a call of their own, element 2^18 the oracle."""
    N = _native()
    a, _ = ab
    n = CHUNK + 3
    x = (np.random.default_rng(18).standard_normal(n) * 100).astype(np.float32)
    rk = bytes(range(9, 41))
    base = 2 ** 33 + 5
    ct, ex, st = _encrypt_dev(a, x, rk, base)
    lo = CHUNK - 2
    big = [t[lo:n].cpu().numpy() for t in (ct, ex, st)]
    del ct, ex, st
    small = [t.cpu().numpy() for t in _encrypt_dev(a, x[lo:n].copy(), rk, base + lo)]
    assert _same(big, small)
    got = N.words_to_ints(big[0].view(np.uint32)[2:3])
    assert (got[0], int(big[1][2])) == O.encrypt_value(x[CHUNK], key4096, O.device_r(rk, base + CHUNK, RBYTES))


# ---------------------------------------------------------------- 10. package level
def test_crt4_package_encryptor_with_explicit_r(monkeypatch, key4096):
    """A key holder's PaillierEncryptor.encrypt(x, random_value=r) on 5 000 elements (above the rows' 4 096): its context
    (a fresh runtime registry) runs the split-pair CRT, builds no fixed-base tables, and the decryptor returns x."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    monkeypatch.setattr(_runtime, "_ctxs", collections.OrderedDict())
    monkeypatch.setattr(_runtime, "_private", collections.OrderedDict())
    pub = PaillierPublicKey(key4096.n)
    pd = PaillierDecryptor(pub, PaillierPrivateKey(pub, key4096.p, key4096.q))
    pe = PaillierEncryptor(pub)
    x = (np.random.default_rng(7).standard_normal(5000) * 100).astype(np.float32)
    r = int.from_bytes(np.random.default_rng(8).bytes(1024), "little") % key4096.nsquare
    ctx = _runtime.context(pub)
    ctx.set_stage_timing(True)
    enc = pe.encrypt(x, random_value=r)
    assert len(ctx.stage_times()) == 3
    ctx.set_stage_timing(False)
    assert ctx.has_private and ctx.pair_paths & 8 and not ctx.fb_ready
    flat = np.asarray(enc).reshape(-1)
    for i in (0, 4999):
        assert (flat[i].ciphertext(False), flat[i].exponent) == O.encrypt_value(x[i], key4096, r), f"element {i}"
    assert np.array_equal(pd.decrypt(enc), x.astype(np.float64))
