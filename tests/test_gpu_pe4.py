"""GPU parity of the public-key encryption on pair groups for n of 2049..4096 bits (kernels_pe4.hpp: k_pe4_pre /
k_pe4_pow / k_pe4_fin, the path of a party that holds only the public key, for calls the row kernel k_pe_w does not
take) against the reference golden vectors (explicit r), the CPU oracle (device ChaCha20 obfuscators) and the
group-engine kernel it replaces (k_encrypt<8>, $FLEXPAI_PAIR=0 in the test build): bit-identical ciphertexts,
exponents, statuses.

The oracle's r^n mod n^2 at 4096 bits takes most of a second on the host, so the cases that compare the same
elements share one set of oracle values (module fixtures), and the array-wide comparisons are against k_encrypt."""
import collections

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

KEY32 = bytes(range(32))
RBYTES = ((4096 + 64 + 31) // 32) * 4        # bytes of the ChaCha20 stream k_encrypt and k_pe4_pre draw


def _native():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def key4096(golden):
    k = golden["keys"]["4096"]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _pub(monkeypatch, n, pair):
    """a (pair): a public context of the product library; b: one of the test build under FLEXPAI_PAIR=0 (k_encrypt);
    both with rows_max 0, so that every call runs the chain under test and not k_pe_w."""
    N = _native()
    monkeypatch.setenv("FLEXPAI_PAIR", "1" if pair else "0")
    ctx = N.Context(n, 0, lib=None if pair else N.load_library(N.XCHECK_LIB_PATH))
    ctx.set_rows_max(0)
    return ctx


@pytest.fixture
def ab(monkeypatch, key4096):
    return _pub(monkeypatch, key4096.n, True), _pub(monkeypatch, key4096.n, False)


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
def test_pe4_path_is_taken(ab, key4096):
    N = _native()
    a, b = ab
    assert a.pair_paths & 4, "the product's public 4096-bit context runs on pair groups"
    assert not b.pair_paths & 4
    x = _mixed(33, 1)
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=3)
    assert _stages(a, x, **kw) == 3, "k_pe4_pre, k_pe4_pow, k_pe4_fin"
    assert _stages(b, x, **kw) == 1, "k_encrypt<8>"
    h = N.Context(key4096.n, 0, key4096.p, key4096.q)
    h.set_rows_max(0)
    h.set_fixed_base(False)
    assert not h.pair_paths & 4, "a key holder's explicit-r / small device-RNG calls stay on k_encrypt<8>"
    assert _stages(h, x, obf_mode=N.PAI_OBF_GIVEN, r=[7 + i for i in range(33)]) == 1


# ---------------------------------------------------------------- 2. goldens
def test_pe4_given_r_matches_reference_goldens(golden, ab):
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


@pytest.fixture(scope="module")
def head_oracle(key4096):
    def ref(x):
        return [O.encrypt_value(x[i], key4096, O.device_r(KEY32, 77 + i, RBYTES)) for i in range(4)]
    return {"f32": ref(X300), "f64": ref(X300.astype(np.float64) * (1.0 + 2.0 ** -40)),
            "i64": ref(np.array([0, -1, 2 ** 40 + 1, -(2 ** 52)], dtype=np.int64))}


@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 33, 300])
def test_pe4_ragged_counts_match_k_encrypt_and_oracle(ab, head_oracle, n):
    """One element, one short of a wave's 8 groups, exactly 8, one over, one short of and one over a block's 32 groups,
    several blocks."""
    N = _native()
    a, b = ab
    x = X300[:n]
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=77)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0][: min(n, 4)])
    for i in range(min(n, 4)):
        assert (got[i], int(ra[1][i])) == head_oracle["f32"][i], f"element {i}"


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_pe4_other_dtypes(ab, head_oracle, kind):
    N = _native()
    a, b = ab
    rng = np.random.default_rng(64)
    if kind == "f64":
        x = rng.standard_normal(33) * 10.0 ** rng.integers(-30, 30, 33)
        x[:4] = X300[:4].astype(np.float64) * (1.0 + 2.0 ** -40)
    else:
        x = rng.integers(-2 ** 53, 2 ** 53, 33, dtype=np.int64)
        x[:4] = [0, -1, 2 ** 40 + 1, -(2 ** 52)]
    kw = dict(obf_mode=N.PAI_OBF_RNG, rng_key=KEY32, index_base=77)
    ra, rb = a.encrypt(x, **kw), b.encrypt(x, **kw)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0][:4])
    for i in range(4):
        assert (got[i], int(ra[1][i])) == head_oracle[kind][i], f"element {i}"


# ---------------------------------------------------------------- 4. edge obfuscators
def test_pe4_edge_obfuscators(ab, key4096):
    """r = 0, 1, 2, n - 1, n, n + 1, multiples of p and q (non-units), n^2 - 1, all-ones words (r >= n^2)."""
    N = _native()
    a, b = ab
    k = key4096
    rs = [0, 1, 2, k.n - 1, k.n, k.n + 1, 5 * k.p, 3 * k.q, k.nsquare - 1, (1 << (32 * a.ct_words)) - 1]
    x = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e30, 3.5, -2.25, 7.0, 0.5], dtype=np.float32)
    ra = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    rb = b.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    for i, r in enumerate(rs):
        assert (got[i], int(ra[1][i])) == O.encrypt_value(x[i], k, r), f"r #{i}"


def test_pe4_one_r_for_all_elements(ab, key4096):
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


# ---------------------------------------------------------------- 5. other moduli
def _modulus(kind):
    """Fixed-seed random odd n (encryption never uses the factors, so these need not be semiprimes)."""
    rng = np.random.default_rng(2049)
    bits = {"2049": 2049, "3072": 3072, "4095": 4095, "4096-top-ones": 4096}[kind]
    v = int.from_bytes(rng.bytes(512), "little") >> (4096 - bits)
    v |= (1 << (bits - 1)) | 1
    if kind == "4096-top-ones":
        v |= ((1 << 64) - 1) << (4096 - 64)
    assert v.bit_length() == bits
    return v


@pytest.mark.parametrize("kind", ["2049", "3072", "4095", "4096-top-ones"])
def test_pe4_other_moduli(monkeypatch, kind):
    """The ends of the range and a modulus with its top 64 bits set: the padding limbs 147..151 and the R >= 2^24 n
    bound at the top."""
    N = _native()
    n = _modulus(kind)
    key = O.Key(n)
    a, b = _pub(monkeypatch, n, True), _pub(monkeypatch, n, False)
    assert a.pair_paths & 4 and not b.pair_paths & 4
    rng = np.random.default_rng(n.bit_length())
    rs = [int.from_bytes(rng.bytes(1024), "little") % (n * n) for _ in range(9)]
    x = _mixed(9, 5)
    ra = a.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    rb = b.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
    assert _same(ra, rb)
    got = N.words_to_ints(ra[0])
    for i, r in enumerate(rs):
        assert (got[i], int(ra[1][i])) == O.encrypt_value(x[i], key, r), f"element {i}"


# ---------------------------------------------------------------- 6. the grid-stride loop
def test_pe4_grid_stride_loop(ab, key4096):
    """40 003 elements: more than the 3 blocks x 256 CUs x 32 groups = 24 576 elements a grid can hold at once (the
    kernels are built for 2 blocks per CU), so every block walks its loop more than once, with a ragged tail."""
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
    d = N.Context(key4096.n, 0, key4096.p, key4096.q)
    val, _, _, _ = d.decrypt(ra[0], ra[1])
    assert np.array_equal(val, x.astype(np.float64))


# ---------------------------------------------------------------- 7. package level
def test_pe4_package_encryptor_without_private_key(monkeypatch, key4096):
    """A party that holds only the public key: its encryptor's context (a fresh runtime registry, so that no private
    key an earlier test registered for this n is attached to it) runs on pair groups; the key holder decrypts."""
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    monkeypatch.setattr(_runtime, "_ctxs", collections.OrderedDict())
    monkeypatch.setattr(_runtime, "_private", collections.OrderedDict())
    pub = PaillierPublicKey(key4096.n)
    pe = PaillierEncryptor(pub)
    x = (np.random.default_rng(7).standard_normal(5000) * 100).astype(np.float32)
    enc = pe.encrypt(x)
    ctx = _runtime.context(pub)
    assert not ctx.has_private and ctx.pair_paths & 4
    pd = PaillierDecryptor(pub, PaillierPrivateKey(pub, key4096.p, key4096.q))
    assert np.array_equal(pd.decrypt(enc), x.astype(np.float64))
