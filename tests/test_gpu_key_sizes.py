"""The key holder's encryption and decryption at the key sizes between the golden ones, bit-exact against the oracle
(oracle/paillier_oracle.py: Python integers, no dependence on the key size).

pai_ctx_set_private picks a kernel family, a limb count and chunk counts per band of key lengths (csrc/flexpai.hip:
setup_crt, setup_fbg, setup_rows4096, setup_crt4, setup_pe*, set_private_impl). Limbs hold LB = 28 bits, a lane 37 limbs
(1036 bits). pb: bits of the larger prime, nb: bits of n, W = ct_words = ceil(2 nb / 32). The map, as the library reported
it on an MI355X (test_key_map asserts it from the inequalities written out in _expect, not from the library):

  key (primes)     sa/sb  kp kd  tpi_e/d  crt  pair  lane  encrypt above the rows      decrypt above the rows    sampler
  K512  (256/256)  19/37   2  1   2/1     yes   7    yes   k_crt_a<19> + b_pair        pair, k_decrypt<1>        refused
  K768  (384/384)  19/37   3  2   2/1     yes   7    yes   as K512                     as K512                   refused
  K1024 (golden)   19/37   4  2   2/1     yes   7    yes   as K512                     as K512                   k_fbs<19>
  K1034 (517/517)  19/37   4  3   2/2     yes   3    yes   as K512                     pair, k_decrypt<2>        refused
  K1035 (518/517)  37/74   3  2   2/2     yes   3    yes   k_crt_a<37> + b_pair        pair, k_decrypt<2>        refused
  K1036 (518/518)  37/74   3  2   4/2     yes   3    yes   as K1035                    as K1035                  refused
  K1536 (768/768)  37/74   3  2   4/2     yes   3    yes   as K1035                    as K1035                  refused
  K2048 (golden)   37/74   4  2   4/2     yes   7    yes   as K1035                    as K1035                  k_fbs<37>
  K2050 (1025/1025) 37/74  -  -   4/2     no    0    no    k_pe_w<148> / k_encrypt<4>  k_decrypt<2> only         none
  K2071 (1036/1035)  -     -  -   4/4     no    0    no    k_pe_w<148> / k_encrypt<4>  k_decrypt<4> only         none
  K2072 (1036/1036) 74/148 3  2   8/4     no    9    no    k_crt4_*                    k_dec4_*, k_decrypt<4>    k_sgp<74>
  K3072 (1536/1536) 74/148 3  2   8/4     no    9    no    as K2072                    as K2072                  k_sgp<74>
  K4096 (golden)   74/148  4  2   8/4     no    9    no    as K2072                    as K2072                  k_sgs<74>
  K1034T (517/517) 19/37   4  3   2/2     yes   3    yes   as K1034                    as K1034                  refused
  K2048T (1024/1024) 37/74 4  2   4/2     yes   7    yes   as K2048                    as K2048                  k_fbs<37>

  K1034T and K2048T are top-heavy: their primes are the two largest below 2^517 and below 2^1024, so p_h and p_h^2 lie
  within a hair of the power of two above them, where K1034 and K2048 meet the pair kernels' bounds (2 pb + 2 = 28 * 37,
  28 * 37 = pb + 12) with primes whose top bits are random.

  sa/sb   limbs of p_h and of p_h^2: the first of (19, 37), (37, 74) with 28 sa >= pb + 2 and 28 sb >= 2 pb + 2 (pb <= 517,
          pb <= 1034); no pair for pb >= 1035, where setup_fbg / setup_rows4096 / setup_crt4 take 74/148 if tpi_e = 8
  kp      chunks of the ciphertext in the pair decryption above the rows: ceil(32 W / 28 sa) (decp_kchunks; dec4_kchunks
          over 74 limbs at 74/148)
  kd      chunks in k_dec_w on the rows: ceil(32 W / 28 sb) (decw_kchunks)
  tpi_e/d lanes of the group engine for n^2 (2 nb + 2 bits) and for decryption (nb + 3 bits)
  crt     PAI_OPT_CRT_AVAILABLE: the lane CRT with the pair bound 28 sa >= pb + 12 met. K2050 finds 37/74 but misses the
          pair bound (1036 < 1037): crt_ok is cleared and the key holder encrypts on the public-key kernels and decrypts
          on k_decrypt<2>. The 74/148 keys report 0 as well: their CRT routes show in pair bit 8 (k_crt4_*) and on the rows.
  pair    PAI_OPT_PAIR: 1 = pair (or split-pair) decryption, 2 = pair CRT stage B, 4 = public-key constants on pairs
          (k_pe1_* for nb <= 1024, k_pe_* for 1537..2048), 8 = k_crt4_*
  lane    PAI_OPT_LANE_DECRYPT
  sampler the fixed-base sampler of device-RNG encryption (fb_plan): the pair tables need W = 2 x the table row (64 or 128
          words: n of 1009..1024 and 2033..2048 bits), so every in-between key is refused and draws r from ChaCha20 on the
          generic route; the 74/148 keys take the split-pair sampler (Shoup rows, k_sgs, only where mu = floor(R^2 / p_h)
          fits 75 limbs: the 4096-bit key). "none": PAI_OPT_FIXED_BASE is 0 from the start.
  On the rows (calls of at most PAI_OPT_ROWS_MAX elements) every key with sa/sb encrypts on k_crt_w<sa, sb> and decrypts
  on k_dec_w<sa, sb>; K2050 and K2071 encrypt on k_pe_w<148>. The kernel names are those of a kernel trace of this module.

Two things the map shows that are easy to misread in the code: K1034 has kd = 3, not the 1024-bit key's 2 (32 * 65 =
2080 > 2 * 1036), and a public-only context of 1537..2032 bits never runs k_pe_*: setup_pe builds its constants (pair
bit 4), but k_pe_fin writes 64-word pairs, so encrypt_route takes k_pe_* and the public fixed-base tables only at 128
ciphertext words (2033..2048 bits); P1537 and P1792 run k_encrypt<4> above the rows.

Explicit r: for a given r every route gives the same bits, so each case runs on the rows, above them, and on the
public-key kernels (set_crt(False)) on and above the rows, every output against the oracle. r^n mod n^2 is the oracle's
pow(r, n, n^2), kept per (key, r) so that the three dtypes, the four routes and the public-only contexts share it; the
number of distinct seeded r falls with the key size (a 4096-bit pow takes 0.5 to 0.9 s), the constructed r stay."""
import math

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
LB, LANE = 28, 37                                   # bn_group.hpp: bits of a limb, limbs of a lane
KMAX_CHUNKS = 5                                     # kernels_crt.hpp
ROWS_MAX = 4096                                     # PAI_OPT_ROWS_MAX's default
# name -> (bits of n, bits of the two primes, first seed tried); None: a golden key
SPECS = {"K512": None, "K768": (768, 384, 384, 1), "K1024": None, "K1034": (1034, 517, 517, 1),
         "K1035": (1035, 518, 517, 1), "K1036": (1036, 518, 518, 1), "K1536": (1536, 768, 768, 1), "K2048": None,
         "K2050": (2050, 1025, 1025, 1), "K2071": (2071, 1036, 1035, 1), "K2072": (2072, 1036, 1036, 1),
         "K3072": (3072, 1536, 1536, 2), "K4096": None,
         "K1034T": "top-heavy", "K2048T": "top-heavy",                        # the two largest primes below 2^517, 2^1024
         "P1537": (1537, 769, 769, 1), "P1792": (1792, 896, 896, 1)}          # public-only contexts (part 5)
BITS = {"K512": 512, "K1024": 1024, "K2048": 2048, "K4096": 4096, "K1034T": 1034, "K2048T": 2048,
        **{k: v[0] for k, v in SPECS.items() if isinstance(v, tuple)}}
HOLDERS = [k for k in SPECS if k.startswith("K")]
PUBLIC = ["K512", "K768", "K1024", "K1035", "K1536", "P1537", "P1792", "K2048"]
# What the library reported on the GPU, per key: (sa, sb), crt_available, pair_paths, lane_decrypt, sampler accepted.
# test_key_map derives the same from the bit lengths (_expect) and compares all three.
REPORTED = {"K512": ((19, 37), True, 7, True, False), "K768": ((19, 37), True, 7, True, False),
            "K1024": ((19, 37), True, 7, True, True), "K1034": ((19, 37), True, 3, True, False),
            "K1035": ((37, 74), True, 3, True, False), "K1036": ((37, 74), True, 3, True, False),
            "K1536": ((37, 74), True, 3, True, False), "K2048": ((37, 74), True, 7, True, True),
            "K2050": ((37, 74), False, 0, False, False), "K2071": (None, False, 0, False, False),
            "K2072": ((74, 148), False, 9, False, True), "K3072": ((74, 148), False, 9, False, True),
            "K4096": ((74, 148), False, 9, False, True),
            "K1034T": ((19, 37), True, 3, True, False), "K2048T": ((37, 74), True, 7, True, True)}


def _native():
    from flex.crypto.paillier import _native
    return _native


def _make_key(name, golden):
    if name == "K512":
        k = next(e for e in golden["keygen"] if e["nb"] == 512 and e["seed"] == 99)
    elif SPECS[name] is None:
        k = golden["keys"][name[1:]]
    elif SPECS[name] == "top-heavy":
        from test_gpu_ops_sizes import _make_key as make      # p and q stepped down from the power of two
        return make(name, golden)
    else:
        nb, pb, qb, seed = SPECS[name]
        while True:                                  # step the seed until n has exactly nb bits
            p, q = O.getprimeover(pb, seed=seed), O.getprimeover(qb, seed=seed + 1000)
            if p != q and (p * q).bit_length() == nb:
                return O.Key(p * q, p, q)
            seed += 1
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


class _Keys:
    """Keys, key-holder contexts and public-only contexts on the product library, and the oracle's r^n mod n^2 per
    (key, r): made on first use and kept for the module."""

    def __init__(self, golden):
        self.golden, self.keys, self.holders, self.publics, self.rn = golden, {}, {}, {}, {}

    def key(self, name):
        if name not in self.keys:
            self.keys[name] = _make_key(name, self.golden)
            assert self.keys[name].n.bit_length() == BITS[name]
        return self.keys[name]

    def holder(self, name):
        if name not in self.holders:
            key = self.key(name)
            self.holders[name] = _native().Context(key.n, 0, key.p, key.q)
        return self.holders[name], self.key(name)

    def public(self, name):
        if name not in self.publics:
            self.publics[name] = _native().Context(self.key(name).n, 0)
        return self.publics[name], self.key(name)

    def r_pow_n(self, key, r):
        k = (key.n, r)
        if k not in self.rn:
            self.rn[k] = pow(r, key.n, key.nsquare)
        return self.rn[k]

    def encrypt(self, x, key, r):
        """O.encrypt_value(x, key, r) with the obfuscator's power taken from the cache: encode, c0 = 1 + n m,
        c0 r^n mod n^2 (O.raw_encrypt's closed form; r = 1 gives c0, as there)."""
        m, e = O.encode(x, key.n, key.max_int)
        return (key.n * m + 1) % key.nsquare * self.r_pow_n(key, r) % key.nsquare, e


@pytest.fixture(scope="module")
def K(golden):
    return _Keys(golden)


def _ceil_div(a, b):
    return -(-a // b)


def _expect(key):
    """The map of the module docstring from the bit lengths alone: the inequalities of setup_crt, setup_fbg,
    setup_rows4096, setup_crt4, setup_pe, setup_pe1, fb_plan and pai_ctx_create, written out."""
    nb = key.n.bit_length()
    bits = sorted((key.p.bit_length(), key.q.bit_length()))
    pb = bits[1]
    W = (2 * nb + 31) // 32
    lane_bits = LB * LANE
    e = {"nb": nb, "ct_words": W, "pt_words": (nb + 31) // 32}
    e["tpi_e"] = next(t for t in (2, 4, 8) if lane_bits * t >= 2 * nb + 2)
    e["tpi_d"] = next(t for t in (1, 2, 4, 8) if lane_bits * t >= nb + 3)
    e["limbs"] = next(((sa, sb) for sa, sb in ((19, 37), (37, 74)) if LB * sa >= pb + 2 and LB * sb >= 2 * pb + 2), None)
    e["pe1"] = nb + 12 <= LB * 37 and W <= 64                     # k_pe1_*: R = 2^1036 >= 2^12 n
    e["pe"] = 1536 < nb and nb + 24 <= LB * 74                    # k_pe_*'s constants: R = 2^2072 >= 2^24 n
    e["kp"] = e["kd"] = 0
    crt = pair = dec4 = crt4 = fbg = sampler = False
    if e["limbs"]:
        sa, sb = e["limbs"]
        e["kd"] = _ceil_div(32 * W, LB * sb)
        # the pair kernels need R = 2^(28 sa) >= 2^12 p_h; without them the lane constants are not used (crt_ok cleared)
        pair = LB * sa >= pb + 12 and e["kd"] <= KMAX_CHUNKS
        crt = pair
        if pair:
            e["kp"] = _ceil_div(32 * W, LB * sa)
        else:
            e["kd"] = 0                                           # k_dec_w's constants exist, nothing runs them
        # fb_plan: Shoup rows on pairs. A ciphertext half is one table row of TW words: W = 2 TW; p_h below 2^(32 PW),
        # above 2^(28 (sa - 1)), R >= 2^12 p_h (FBP_PB + 1), q < 2 p
        tw = 32 if sb == 37 else 64
        sampler = (pair and W == 2 * tw and 2 * pb <= 32 * tw and bits[1] <= 16 * tw and bits[0] > LB * (sa - 1)
                   and pb + 12 <= LB * sa and key.q < 2 * key.p)
    else:
        fbg = LB * 4 * LANE >= 2 * pb + 4 and e["tpi_e"] == 8     # p_h^2 on 4 lanes of the group engine
        if fbg:
            e["limbs"] = (74, 148)
        kp4 = _ceil_div(32 * W, LB * 74)
        dec4 = fbg and pb + 24 <= LB * 74 and kp4 <= 4 and e["tpi_d"] == 4
        rows4 = fbg and pb + 2 <= LB * 74 and _ceil_div(32 * W, LB * 148) <= KMAX_CHUNKS
        crt4 = rows4 and pb + 24 <= LB * 74
        if dec4:
            e["kp"] = kp4
        if rows4:
            e["kd"] = _ceil_div(32 * W, LB * 148)
        # the split-pair sampler: p_h on 76 limbs with R >= 2^24 p_h, at most 74 non-zero limbs and 64 words
        sampler = fbg and pb + 24 <= LB * 76 and pb <= LB * 74 and pb <= 2048 and key.q < 2 * key.p
    e["crt_available"] = crt
    e["lane_decrypt"] = pair
    e["pair_paths"] = (1 if pair or dec4 else 0) | (2 if pair else 0) | (4 if e["pe"] or e["pe1"] else 0) | (8 if crt4 else 0)
    e["fixed_base_untried"] = crt or fbg                          # PAI_OPT_FIXED_BASE before the first build
    e["sampler"] = sampler
    return e


# --------------------------------------------------------------------------- 1. the map
@pytest.mark.parametrize("name", HOLDERS)
def test_key_map(K, name):
    ctx, key = K.holder(name)
    e = _expect(key)
    got = {"nb": ctx.key_bits, "ct_words": ctx.ct_words, "pt_words": ctx.pt_words, "crt_available": ctx.crt_available,
           "pair_paths": ctx.pair_paths, "lane_decrypt": ctx.lane_decrypt}
    print(f"{name}: p/q {key.p.bit_length()}/{key.q.bit_length()} expect {e} reports {got}")
    assert e["nb"] == BITS[name]
    for k, v in got.items():
        assert v == e[k], f"{name} {k}: the context reports {v}, the inequalities give {e[k]}"
    assert (e["limbs"], e["crt_available"], e["pair_paths"], e["lane_decrypt"], e["sampler"]) == REPORTED[name]
    # the seams the table rests on
    nb, pb = e["nb"], max(key.p.bit_length(), key.q.bit_length())
    if name in ("K1034", "K1034T"):
        assert 2 * pb + 2 == LB * 37 and (e["tpi_d"], e["kd"]) == (2, 3)
    if name == "K1035":
        assert 2 * nb + 2 == 2 * LB * LANE and e["tpi_e"] == 2 and e["limbs"] == (37, 74)
    if name == "K1036":
        assert e["tpi_e"] == 4
    if name in ("K2048", "K2048T"):
        assert LB * 37 == pb + 12
    if name in ("K1034T", "K2048T"):                 # top-heavy: p_h^2 within 2^-500 of the power of two above it
        assert all(h.bit_length() == pb and (1 << 2 * pb) - h * h < 1 << (2 * pb - 500) for h in (key.p, key.q))
    if name == "K2050":
        assert e["limbs"] == (37, 74) and LB * 37 < pb + 12
    if name == "K2071":
        assert e["limbs"] is None and e["tpi_e"] == 4 and e["ct_words"] == 130
    if name == "K2072":
        assert (e["tpi_e"], e["tpi_d"], e["kp"], e["kd"]) == (8, 4, 3, 2)


# --------------------------------------------------------------------------- 2. explicit r
def _crt(a, b, key):
    """The residue mod n that is a mod p and b mod q."""
    return (b + key.q * ((a - b) * key.q_inverse % key.p)) % key.n


def _r_list(key, count):
    """`count` obfuscators: the constructed ones, then seeded ones, repeated. All units mod n."""
    n, p, q = key.n, key.p, key.q
    nb = n.bit_length()
    a, b = 2 + O.golden_r(n, 71, 0) % (q - 2), 2 + O.golden_r(n, 71, 1) % (p - 2)
    made = [_crt(1, a, key), _crt(p - 1, a, key),          # stage A's result mod p is 1 / p - 1
            1, 2, n - 1, n - 2, 1 << (nb - 1),
            _crt(b, 1, key), _crt(b, q - 1, key),          # ... and mod q
            0x5A5A5A5]                                     # below p: one limb
    seeded = 48 if nb <= 1100 else 20 if nb <= 2100 else 2
    rs = made + [O.golden_r(n, 4711, i) for i in range(seeded)]
    assert all(0 < r < n and math.gcd(r, n) == 1 for r in rs) and made[9] < min(p, 1 << LB)
    assert made[0] % p == 1 and made[1] % p == p - 1 and made[7] % q == 1 and made[8] % q == q - 1
    return [rs[i % len(rs)] for i in range(count)]


def _plain(dt, count, seed):
    """Plaintexts of one dtype: zero, tiny values on both sides of the encoder's 1e-200 cut, auto exponents far below
    and far above 0, the int64 extremes; random values between them. The specials come round twice, so each meets two
    different obfuscators."""
    rng = np.random.default_rng(seed)
    if dt == np.int64:
        x = rng.integers(-(2 ** 63), 2 ** 63 - 1, count, dtype=np.int64, endpoint=True)
        sp = [2 ** 63 - 1, -(2 ** 63), 0, 1, -1, -(2 ** 63) + 1, 2 ** 62, -(2 ** 62), 12345, -99991, 2 ** 53 + 1, 16, -16]
    elif dt == np.float32:
        x = (rng.standard_normal(count) * 10.0 ** rng.integers(-30, 31, count)).astype(np.float32)
        sp = [1e30, 0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, -1e30, 1e-30, -1e-30, 3.4028235e38, 1.0, -1.5, 0.1, 16.0,
              1.1754944e-38]
    else:
        x = rng.standard_normal(count) * 10.0 ** rng.integers(-30, 31, count)
        sp = [1e30, 0.0, -0.0, 1e-201, -1e-201, 0.99e-200, 1e-200, 1.01e-200, 1e-199, -1e-199, -1e30, 1e-30, -1e-30, 5e-324,
              1.0, -1.5, 0.1, 16.0, 2.0 ** -1000, 1.7976931348623157e308, 2.0 ** 52 + 0.5]
    sp = np.array(sp, dtype=dt)
    for j in range(2 * len(sp)):
        if 3 * j < count:
            x[3 * j] = sp[j % len(sp)]
    return x


def _py(v, dt):
    return int(v) if dt == np.int64 else (np.float32(v) if dt == np.float32 else float(v))


def _same(ct, ex, want, what):
    got = list(zip(_native().words_to_ints(ct), (int(e) for e in ex)))
    assert len(got) == len(want), what
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{what}: {len(bad)} of {len(want)} outputs differ from the oracle, first at {bad[:8]}"


class _Routes:
    """Context options for one route, put back afterwards (the contexts are shared by the module)."""

    def __init__(self, ctx, rows_max=None, crt4_min=None, crt=None, lane_decrypt=None):
        self.ctx, self.want = ctx, (rows_max, crt4_min, crt, lane_decrypt)

    def __enter__(self):
        c = self.ctx
        self.was = (c.rows_max, c.crt4_min, c.crt_enabled, None)
        rows_max, crt4_min, crt, lane = self.want
        if rows_max is not None:
            c.set_rows_max(rows_max)
        if crt4_min is not None:
            c.set_crt4_min(crt4_min)
        if crt is not None:
            c.set_crt(crt)
        if lane is not None:
            c.set_lane_decrypt(lane)
        return c

    def __exit__(self, *exc):
        c = self.ctx
        c.set_rows_max(self.was[0])
        c.set_crt4_min(self.was[1])
        c.set_crt(self.was[2])
        if self.want[3] is not None:
            c.set_lane_decrypt(True)
        return False


ENC_ROUTES = {"rows": {}, "above": {"rows_max": 0, "crt4_min": 0}, "public": {"crt": False},
              "public-above": {"crt": False, "rows_max": 0}}
COUNTS = (1, 33, 257)       # ragged against the 16-lane rows and the 32 and 64 groups per block


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int64])
@pytest.mark.parametrize("name", HOLDERS)
def test_given_r_encrypt(K, name, dt):
    N = _native()
    ctx, key = K.holder(name)
    assert ctx.rows_max == ROWS_MAX and ctx.crt_enabled
    nmax = max(COUNTS)
    x = _plain(dt, nmax, key.n.bit_length() + np.dtype(dt).num)
    rs = _r_list(key, nmax)
    want = [K.encrypt(_py(x[i], dt), key, rs[i]) for i in range(nmax)]
    for i in (0, 4, nmax - 1):
        assert want[i] == O.encrypt_value(_py(x[i], dt), key, rs[i])
    for route, opts in ENC_ROUTES.items():
        with _Routes(ctx, **opts):
            for n in COUNTS:
                ct, ex, st = ctx.encrypt(x[:n], obf_mode=N.PAI_OBF_GIVEN, r=rs[:n])
                assert not st.any(), (name, route, n)
                _same(ct, ex, want[:n], f"{name} {np.dtype(dt).name} {route} N={n}")
    assert ctx.rows_max == ROWS_MAX and ctx.crt_enabled


# --------------------------------------------------------------------------- 3. decryption
def _decrypt_inputs(K, key, W):
    """(ciphertexts, exponents, indices of the constructed non-units). First the plaintexts of every decode branch
    (tests/test_gpu_dec_lane.py::test_lane_decrypt_decode_statuses, scaled to the key) encrypted by the oracle, then the
    edge ciphertexts of test_lane_decrypt_edge_ciphertexts, then random words."""
    n, mx, nb = key.n, key.max_int, key.n.bit_length()
    wide = (1 << 1030) + 1 if nb > 1033 else (1 << (nb - 324)) + 1     # wider than 1024 bits where n / 3 allows
    ms = [0, 1, 5, mx, mx + 1, n - mx, n - mx - 1, n - 1, n // 2, (1 << 53) + 1, (1 << 64) + 3,
          ((1 << 54) + 3) << 60, n - ((1 << 63) - 1), n - (1 << 63), wide]
    es = [0, -1, 3, 1, 0, 2, -3, 5, 1, 0, -2, 7, 0, 0, 260]
    assert wide <= mx and all(0 <= m < n for m in ms)
    rs = [O.golden_r(n, 4711, i % 2) for i in range(len(ms))]          # seeded obfuscators, their powers shared with part 2
    cs = [(n * m + 1) % key.nsquare * K.r_pow_n(key, r) % key.nsquare for m, r in zip(ms, rs)]
    assert cs[1] == O.raw_encrypt(1, key, rs[1]) and cs[7] == O.raw_encrypt(n - 1, key, rs[7])
    top = (1 << (32 * W)) - 1
    p, q = key.p, key.q
    edge = [0, 1, 2, p, q, 3 * p, n, key.psquare, key.qsquare, key.nsquare - 1, key.nsquare, key.nsquare + 12345,
            top, top - 1, p * p * 7 + q, (n + 1) % key.nsquare, pow(n + 1, 5, key.nsquare)]
    nonunit = [len(cs) + i for i in (0, 3, 4, 5, 6, 7, 8, 10)]         # 0 and the multiples of p or q
    rng = np.random.default_rng(nb)
    # (a 4096-bit raw_decrypt takes 0.25 s in the oracle: the random tail is cut there, the constructed ones stay)
    rnd = [int.from_bytes(rng.bytes(4 * W), "little") for _ in range(40 if nb <= 2100 else 8 if nb <= 3100 else 4)]
    assert all(math.gcd(c, n) == 1 for c in rnd), "a random ciphertext shares a factor with n"
    cs = cs + edge + rnd
    assert max(cs) <= top
    assert [i for i, c in enumerate(cs) if math.gcd(c, n) != 1] == nonunit
    ex = es + [(i % 7) - 2 for i in range(len(edge) + len(rnd))]
    return cs, np.array(ex, dtype=np.int32), nonunit, [m % n for m in ms]


def _check_decode(N, res, raws, ex, key, idx, what):
    """The exact status, the bits of the value and the mantissa follow the oracle's decode of the plaintext
    (codec_edges.expect_decode: which OverflowError, EL_INT against EL_INT_BIG, the sign of zero)."""
    from codec_edges import expect_decode
    val, mant, st, _ = res
    bits = np.ascontiguousarray(val, dtype=np.float64).view(np.uint64)
    for i in idx:
        want = expect_decode(raws[i], int(ex[i]), key.n, key.max_int)
        assert st[i] == want.st, f"{what} element {i}: status {st[i]}, expected {want.st}"
        if want.bits is not None:
            assert int(bits[i]) == want.bits, f"{what} element {i}: value {float(val[i]).hex()}"
        if want.mant is not None:
            assert int(mant[i]) == want.mant, f"{what} element {i}"


@pytest.mark.parametrize("name", HOLDERS)
def test_decrypt_routes(K, name):
    N = _native()
    ctx, key = K.holder(name)
    e = _expect(key)
    cs, ex, nonunit, plain = _decrypt_inputs(K, key, ctx.ct_words)
    ct = N.ints_to_words(cs, ctx.ct_words)
    want_raw = [O.raw_decrypt(c, key) for c in cs]
    assert want_raw[:len(plain)] == plain
    unit = np.ones(len(cs), dtype=bool)
    unit[nonunit] = False
    every, units = range(len(cs)), [int(i) for i in np.flatnonzero(unit)]
    assert ctx.lane_decrypt == e["lane_decrypt"]
    res = {}
    for route, opts in (("rows", {}), ("above", {"rows_max": 0}), ("group", {"lane_decrypt": False})):
        with _Routes(ctx, **opts):
            assert (ctx.pair_paths & 1) == (e["pair_paths"] & 1 if route != "group" else 0)
            res[route] = ctx.decrypt(ct, ex, want_raw=True)
        # the pair kernels follow the reference on every ciphertext; the group engine's k_decrypt wherever c is a unit
        # (it does not special-case c == 0 mod p, where the reference's floor division gives L = -1)
        idx = every if (route != "group" and e["pair_paths"] & 1) else units
        raw = N.words_to_ints(res[route][3])
        bad = [i for i in idx if raw[i] != want_raw[i]]
        assert not bad, f"{name} {route}: plaintexts differ from the oracle at {bad[:8]}"
        _check_decode(N, res[route], want_raw, ex, key, idx, f"{name} {route}")
    assert ctx.pair_paths == e["pair_paths"] and ctx.rows_max == ROWS_MAX
    for route in ("above", "group"):
        for x, y in zip(res["rows"], res[route]):
            assert np.array_equal(np.asarray(x)[unit].view(np.uint8), np.asarray(y)[unit].view(np.uint8)), (name, route)


# --------------------------------------------------------------------------- 4. device RNG
RNG_KEY = bytes(range(7, 39))
RNG_BASE = 2 ** 33 + 5
RNG_CHECK = (0, 66, 100, 199)


def _rng_values():
    rng = np.random.default_rng(200)
    x = (rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200)).astype(np.float32)
    x[::17] = 0.0
    return x


def _generic_r(key, i):
    """The obfuscator of the generic route: nb + 64 bits of the element's ChaCha20 stream, used mod n."""
    return O.device_r(RNG_KEY, RNG_BASE + i, ((key.n.bit_length() + 64 + 31) // 32) * 4) % key.n


@pytest.mark.parametrize("name", HOLDERS)
def test_device_rng_encrypt(K, name):
    N = _native()
    ctx, key = K.holder(name)
    e = _expect(key)
    ctx.set_fb_window(8)
    if not ctx.fb_ready:
        assert ctx.fixed_base == e["fixed_base_untried"]
        try:
            ctx.prepare_fixed_base()
        except N.NativeError:
            pass
    accepted = ctx.fb_ready
    assert accepted == e["sampler"], f"{name}: the sampler {'accepts' if accepted else 'refuses'} the key"
    assert ctx.fixed_base == accepted
    x = _rng_values()
    ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=RNG_KEY, index_base=RNG_BASE)
    assert not st.any() and ctx.fb_ready == accepted
    print(f"{name}: sampler {'accepted' if accepted else 'refused'}, fb_pair {ctx.fb_pair}, split_sampler {ctx.split_sampler}")
    got = N.words_to_ints(ct)
    params = ctx.fixed_base_info() if accepted else None
    for i in RNG_CHECK:
        want = (O.fb_encrypt_value(x[i], key, RNG_KEY, RNG_BASE + i, params) if accepted
                else O.encrypt_value(x[i], key, _generic_r(key, i)))
        assert (got[i], int(ex[i])) == want, f"{name} element {i} ({'sampler' if accepted else 'generic'})"
    val = ctx.decrypt(ct, ex)[0]
    assert np.array_equal(val, x.astype(np.float64))    # (a float32 encodes exactly; exponents <= 0 decode with EL_INT)


# --------------------------------------------------------------------------- 5. public-only contexts
@pytest.mark.parametrize("name", PUBLIC)
def test_public_only_encrypt(K, name):
    """Above the rows: k_pe1_* (nb <= 1024), k_pe_* (128 ciphertext words), else k_encrypt; every output. Then the rows
    (k_pe_w) on the same inputs."""
    N = _native()
    ctx, key = K.public(name)
    nb = key.n.bit_length()
    W = (2 * nb + 31) // 32
    pe1, pe = nb + 12 <= LB * 37 and W <= 64, 1536 < nb and nb + 24 <= LB * 74
    assert (ctx.key_bits, ctx.ct_words, ctx.pt_words) == (nb, W, (nb + 31) // 32)
    assert ctx.pair_paths == (4 if pe1 or pe else 0) and not ctx.crt_available
    n = 257
    x = _plain(np.float64, n, nb + 5)
    rs = _r_list(key, n)
    want = [K.encrypt(float(x[i]), key, rs[i]) for i in range(n)]
    assert want[3] == O.encrypt_value(float(x[3]), key, rs[3])
    for rows_max in (0, ROWS_MAX):
        with _Routes(ctx, rows_max=rows_max):
            ct, ex, st = ctx.encrypt(x, obf_mode=N.PAI_OBF_GIVEN, r=rs)
        assert not st.any()
        _same(ct, ex, want, f"public {name} rows_max={rows_max}")
    # the public fixed bases: pfb_supported's condition is k_pe's constants and 128 ciphertext words
    assert ctx.public_fixed_base == (pe and W == 128)
    if name in ("P1537", "P1792"):
        assert not ctx.public_fixed_base
        with pytest.raises(N.NativeError, match="2033..2048 bits"):
            ctx.prepare_public_fixed_base()
        assert not ctx.pfb_ready
        xr = _rng_values()
        ct, ex, st = ctx.encrypt(xr, obf_mode=N.PAI_OBF_RNG, rng_key=RNG_KEY, index_base=RNG_BASE)
        got = N.words_to_ints(ct)
        for i in RNG_CHECK:
            assert (got[i], int(ex[i])) == O.encrypt_value(xr[i], key, _generic_r(key, i)), f"{name} element {i}"


# --------------------------------------------------------------------------- 6. the package
@pytest.mark.parametrize("n_length", [768, 1536, 3072])
def test_package_round_trip(n_length, monkeypatch):
    """generate_paillier_encryptor_decryptor at sizes the device prime search does not cover (384-, 768- and 1536-bit
    primes: the host search), then encrypt, a + b, a * 3.5 and decrypt: the key is the oracle's, the sums and products
    are the oracle's bits on the ciphertexts the encryptor made, the decrypted values the oracle's decode."""
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    monkeypatch.setenv("FLEXPAI_FB_WINDOW", "8")     # the 3072-bit key's sampler tables stay small
    pe, pd = generate_paillier_encryptor_decryptor(n_length, seed=5)
    n, p, q = O.generate_keypair(n_length, seed=5)
    assert (pe.pub_key.n, pd.priv_key.p, pd.priv_key.q) == (n, p, q) and n.bit_length() == n_length
    key = O.Key(n, p, q)
    rng = np.random.default_rng(n_length)
    x = rng.standard_normal(100) * 10.0 ** rng.integers(-8, 9, 100)
    y = rng.standard_normal(100) * 10.0 ** rng.integers(-8, 9, 100)
    x[::9] = 0.0
    a, b = pe.encrypt(x), pe.encrypt(y)

    def pairs(arr):
        return [(c.ciphertext(False), c.exponent) for c in np.asarray(arr).reshape(-1)]

    ca, cb = pairs(a), pairs(b)
    s, m = a + b, a * 3.5
    want_s = [O.add_k([ca[i][0], cb[i][0]], [ca[i][1], cb[i][1]], key) for i in range(100)]
    want_m = [O.mul_scalar(ca[i][0], ca[i][1], 3.5, key) for i in range(100)]
    assert pairs(s) == want_s and pairs(m) == want_m
    da, ds, dm = pd.decrypt(a), pd.decrypt(s), pd.decrypt(m)
    # the plaintexts the oracle's operations hold, decoded by the oracle: every element (a float64 of 53 bits is rounded
    # to the 50..53 bits its exponent leaves, so a decrypts to decode(encode(x)), not always to x)
    for i in range(100):
        (ma, ea), (mb, eb), (m35, e35) = (O.encode(float(v), n, key.max_int) for v in (x[i], y[i], 3.5))
        E = max(ea, eb)
        assert float(da[i]) == O.decode(ma, ea, n, key.max_int) and abs(float(da[i]) - x[i]) <= abs(x[i]) * 2.0 ** -49, i
        assert float(ds[i]) == O.decode((ma * 16 ** (E - ea) + mb * 16 ** (E - eb)) % n, E, n, key.max_int), i
        assert float(dm[i]) == O.decode(ma * m35 % n, ea + e35, n, key.max_int), i
    # ... and the oracle's own decryption of its ciphertexts (a 3072-bit raw_decrypt takes 0.1 s: every fifth there)
    for i in range(0, 100, 1 if n_length < 1024 else 2 if n_length < 2048 else 5):
        assert float(da[i]) == O.decrypt_value(*ca[i], key), i
        assert float(ds[i]) == O.decrypt_value(*want_s[i], key), i
        assert float(dm[i]) == O.decrypt_value(*want_m[i], key), i
