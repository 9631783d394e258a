"""PAI_OPT_PRIME_LIMBS = 1: the 56-limb split-pair kernels (k_crt4_*<56>, k_dec4_*<56>) and rows (k_crt_w<56, 112>,
k_dec_w<56, 112>) of a key holder whose larger prime has 1036..1556 bits, against the oracle (Python integers) and, bit for
bit, against a context of the same key with the option at 0 (the 74-limb kernels). Keys: 3072 (1536/1536); the band's
edges 2072 (1036/1036) and 3112 (1556/1556: 28 * 56 = pb + 12); 3114 (1557/1557), just outside, which reads back 0 and
runs on 74; K3072T, the two largest primes below 2^1536. Counts: 1, one block of 128 lane pairs - 1 / + 0 / + 1, and 300
(three blocks of pairs, two of stage A's 256 lanes, ragged). On the parent commit set_prime_limbs raises (unknown
option), so every test here fails there."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
KEYS = {"K3072": (1536, 56), "K2072": (1036, 56), "K3112": (1556, 56), "K3114": (1557, 0), "K3072T": (1536, 56)}
COUNTS = (1, 127, 128, 129, 300)
PATHS = {"above": (0, 0), "rows": (4096, 128)}          # PAI_OPT_ROWS_MAX, PAI_OPT_CRT4_MIN
EDGES = [0, 1, -1, 2 ** 63 - 1, -(2 ** 63)]             # the int64 encoder's edges; +-max_int go through encrypt_big


def _native():
    from flex.crypto.paillier import _native
    return _native


def _make_key(name):
    pb = KEYS[name][0]
    if name.endswith("T"):
        from test_gpu_ops_sizes import _prime_below
        q = _prime_below(1 << pb)
        p = _prime_below(q)
        return O.Key(p * q, p, q)
    seed = pb
    while True:                                          # step the seed until both primes and n have their full length
        p, q = O.getprimeover(pb, seed=seed), O.getprimeover(pb, seed=seed + 1000)
        if p != q and p.bit_length() == q.bit_length() == pb and (p * q).bit_length() == 2 * pb:
            return O.Key(p * q, p, q)
        seed += 1


class _Case:
    """One key: its two contexts, the obfuscators with the oracle's r^n mod n^2 (one pow each), the expected ciphertexts."""

    def __init__(self, name):
        N = _native()
        self.key = key = _make_key(name)
        self.ctx = {}
        for opt in (1, 0):
            c = self.ctx[opt] = N.Context(key.n, 0)
            c.set_prime_limbs(bool(opt))
            c.set_private(key.p, key.q)
        n, n2 = key.n, key.nsquare
        self.rs = [1, 2, n - 1, key.p, O.golden_r(n, 4711, 0)]     # r = p: zero residue mod p^2
        rn = [pow(r, n, n2) for r in self.rs]
        nmax = max(COUNTS)
        self.x = np.array([EDGES[i % 5] for i in range(nmax)], dtype=np.int64)
        self.r = [self.rs[(i // 5) % 5] for i in range(nmax)]
        self.want = [((n * (int(v) % n) + 1) % n2 * rn[(i // 5) % 5] % n2, 0) for i, v in enumerate(self.x)]
        # +-max_int, or the widest magnitude a PAI_BIG operand carries (ct_words // 2 words: one short at K3112, K3114)
        top = min(key.max_int, (1 << 32 * ((2 * n.bit_length() + 31) // 32 // 2)) - 1)
        assert top == key.max_int or name in ("K3112", "K3114")
        self.big = [top, -top] * 5
        self.big_r = [self.rs[i // 2] for i in range(10)]
        self.want_big = [((n * (v % n) + 1) % n2 * rn[i // 2] % n2, 0) for i, v in enumerate(self.big)]
        assert self.want[8] == O.encrypt_value(int(self.x[8]), key, self.r[8])
        # decryption inputs: c = 1, n^2 - 1, raw encryptions of 0, n - 1 and max_int, then the encryptions above
        sp = [1, n2 - 1] + [(n * m + 1) % n2 * rn[4] % n2 for m in (0, n - 1, key.max_int)]
        self.cs = sp + [c for c, _ in self.want_big + self.want]
        raw = {}                                         # the oracle's decryption, once per distinct non-unit
        self.raw = [0, O.raw_decrypt(n2 - 1, key), 0, n - 1, key.max_int]
        for (c, _), m in zip(self.want_big + self.want, self.big + [int(v) for v in self.x]):
            if c % key.p == 0 and c not in raw:
                raw[c] = O.raw_decrypt(c, key)
            self.raw.append(raw.get(c, m % n))           # a unit decrypts to the plaintext that went in
        assert self.raw[4] == O.raw_decrypt(self.cs[4], key) and self.raw[20] == O.raw_decrypt(self.cs[20], key)
        self.ex = np.array([(i % 5) - 2 for i in range(len(self.cs))], dtype=np.int32)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(name)
        return made[name]
    return get


def _with_path(ctx, path):
    ctx.set_rows_max(PATHS[path][0])
    ctx.set_crt4_min(PATHS[path][1])
    return ctx


@pytest.mark.parametrize("name", KEYS)
def test_read_back(cases, name):
    N, k = _native(), cases(name)
    on, off = k.ctx[1], k.ctx[0]
    assert (on.prime_limbs, off.prime_limbs) == (KEYS[name][1], 0)
    assert on.pair_paths == off.pair_paths == 9         # split-pair decryption and CRT either way
    with pytest.raises(N.NativeError, match="before pai_ctx_set_private"):
        on.set_prime_limbs(False)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", KEYS)
def test_encrypt(cases, name, path):
    N, k = _native(), cases(name)
    on, off = _with_path(k.ctx[1], path), _with_path(k.ctx[0], path)
    for n in COUNTS:
        got = on.encrypt(k.x[:n], obf_mode=N.PAI_OBF_GIVEN, r=k.r[:n])
        assert not got[2].any()
        assert list(zip(N.words_to_ints(got[0]), (int(e) for e in got[1]))) == k.want[:n], (name, path, n)
        ref = off.encrypt(k.x[:n], obf_mode=N.PAI_OBF_GIVEN, r=k.r[:n])
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (name, path, n)
    x, neg, wide = N.big_operand(np.array(k.big, dtype=object), on.ct_words)
    got = on.encrypt_big(x, neg, N.PAI_OBF_GIVEN, r=k.big_r)
    assert wide is None and not got[2].any()
    assert list(zip(N.words_to_ints(got[0]), (int(e) for e in got[1]))) == k.want_big, (name, path)
    assert all(np.array_equal(a, b) for a, b in zip(got, off.encrypt_big(x, neg, N.PAI_OBF_GIVEN, r=k.big_r)))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", KEYS)
def test_decrypt(cases, name, path):
    from test_gpu_key_sizes import _check_decode
    N, k = _native(), cases(name)
    on, off = _with_path(k.ctx[1], path), _with_path(k.ctx[0], path)
    ct = N.ints_to_words(k.cs, on.ct_words)
    for n in COUNTS + (len(k.cs),):
        got = on.decrypt(ct[:n], k.ex[:n], want_raw=True)
        assert N.words_to_ints(got[3]) == k.raw[:n], (name, path, n)
        _check_decode(N, got, k.raw, k.ex, k.key, range(n), f"{name} {path} N={n}")
        ref = off.decrypt(ct[:n], k.ex[:n], want_raw=True)
        for a, b in zip(got, ref):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), (name, path, n)
