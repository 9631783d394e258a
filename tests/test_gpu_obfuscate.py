"""Batched re-randomisation of ciphertext arrays: pai_obfuscate[_dev] (csrc/kernels_obf.hpp: k_obf_mul over the r^n of
the encrypt chains) and its path up to PaillierArray / CiphertextBuffer.

* the reference's apply_obfuscation(c, pub_key, r) bit for bit (tests/golden/paillier_golden_obf.json);
* ragged counts with an explicit r per element against c * pow(r, n, n^2) % n^2;
* the bits contract of include/flexpai.h under device RNG, on every encrypt route: out = c * E0 mod n^2 with E0 the
  encryption of int64 zeros on an identically prepared second context;
* slicing (PAI_OPT_OBF_CHUNK), call splitting, the device entry point, the package layers.

Python's pow costs 0.74 s per r^n at 4096 bits (0.1 s at 2048), so the tests keep literal pow calls to a few per case:
test 2 draws r_i = g^i and the inputs' obfuscators h^i, whose n-th powers follow from ONE pow each by a recurrence of
products (pow(g^i, n, n^2) = pow(g, n, n^2)^i), and checks the recurrence against literal pow and O.encrypt_value on
sampled elements; the sampled checks of test 3 take r^n from the package's GMP binding, and one element per case from
pow itself.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1024, 2048, 4096)
RK = bytes(range(100, 132))
BASE = 7


def _native():
    from flex.crypto.paillier import _native
    return _native


def _powmod(a, b, m):
    from flex.crypto.paillier import _bigint
    return _bigint.powmod(a, b, m)


@pytest.fixture(scope="module")
def golden_obf():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_obf.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def keys(golden):
    out = {}
    for nb in NBS:
        k = golden["keys"][str(nb)]
        out[nb] = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    return out


@pytest.fixture(scope="module")
def pfb_bases(golden_pfb):
    k = golden_pfb["keys"]["2048"]
    return int(k["n"], 16), [int(b, 16) for b in k["bases"]]


class _Ctxs:
    """Contexts by (nb, kind, slot), made on first use and kept for the module. slot 0 and 1 of a kind are prepared
    identically: the second one encrypts the zeros of the bits contract."""

    def __init__(self, keys, pfb_bases):
        self.keys, self.pfb_bases, self.cache = keys, pfb_bases, {}

    def get(self, nb, kind, slot=0):
        k = (nb, kind, slot)
        if k not in self.cache:
            self.cache[k] = self._make(nb, kind)
        return self.cache[k]

    def _make(self, nb, kind):
        N = _native()
        key = self.keys[nb]
        if kind == "holder_sampler":        # fixed-base tables resident
            c = N.Context(key.n, 0, key.p, key.q)
            c.set_fb_window(12)             # small tables: quick to build; the window does not change the bits
            c.prepare_fixed_base()
            assert c.fb_ready
        elif kind == "holder":              # the key holder's generic chains
            c = N.Context(key.n, 0, key.p, key.q)
            c.set_fixed_base(False)
        elif kind == "public":              # the public-key chains
            c = N.Context(key.n, 0)
            c.set_public_fixed_base(False)
        elif kind == "public_sampler":      # public fixed-base tables resident (2048-bit n)
            n, bases = self.pfb_bases
            assert n == key.n
            c = N.Context(key.n, 0)
            c.set_public_bases(bases)
            c.set_pfb_window(12)
            c.prepare_public_fixed_base()
            assert c.pfb_ready
        else:
            raise KeyError(kind)
        return c


@pytest.fixture(scope="module")
def ctxs(keys, pfb_bases):
    return _Ctxs(keys, pfb_bases)


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
    x[::7] = 0.0
    return x


def _inputs(ctx, key, n, seed):
    """n ciphertexts (words, exponents, ints) encrypted on the device under explicit obfuscators (that path is pinned to
    the reference by test_gpu_native.py)."""
    N = _native()
    rs = [O.golden_r(key.n, 900 + seed, i) for i in range(n)]
    ct, ex, st = ctx.encrypt(_mixed(n, seed), obf_mode=N.PAI_OBF_GIVEN, r=rs)
    assert not st.any()
    return ct, ex, N.words_to_ints(ct)


def _sample(n, k=8):
    return sorted({int(v) for v in np.linspace(0, n - 1, min(n, k))})


# ---------------------------------------------------------------- 1. the reference's apply_obfuscation
@pytest.mark.parametrize("party", ["holder", "public"])
@pytest.mark.parametrize("nb", NBS)
def test_reference_golden(ctxs, golden_obf, nb, party):
    N = _native()
    ctx = ctxs.get(nb, party)
    recs = golden_obf["cases"][str(nb)]
    ct = N.ints_to_words([int(r["c"], 16) for r in recs], ctx.ct_words)
    out = ctx.obfuscate(ct, obf_mode=N.PAI_OBF_GIVEN, r=[int(r["r"], 16) for r in recs])
    got = N.words_to_ints(out)
    for i, rec in enumerate(recs):
        assert hex(got[i]) == rec["out"], (i, rec["kind"])


# ---------------------------------------------------------------- 2. ragged counts, explicit r, Python pow
@pytest.fixture(scope="module")
def pools(keys):
    """Per key size: 300 inputs c_i = O.encrypt_value(x_i, key, h^i) and obfuscators r_i = g^i with r_i^n, by the
    recurrence of the module docstring; element 299 (and 2, below 4096 bits) is checked against the literal formulas."""
    out = {}

    def make(nb):
        key = keys[nb]
        n, nsq = key.n, key.nsquare
        g, h = O.golden_r(n, 31, 0), O.golden_r(n, 32, 0)
        G, H = pow(g, n, nsq), pow(h, n, nsq)
        x = _mixed(300, nb)
        rs, rns, cs = [], [], []
        r, rn, hi, hn = 1, 1, 1, 1
        for i in range(300):
            rs.append(r)
            rns.append(rn)
            m, _ = O.encode(np.float64(x[i]), n, key.max_int)
            cs.append((n * m + 1) % nsq * hn % nsq)
            if i in ((2, 299) if nb < 4096 else (299,)):
                assert rn == pow(r, n, nsq)
                assert cs[i] == O.encrypt_value(np.float64(x[i]), key, hi)[0]
            r, rn, hi, hn = r * g % nsq, rn * G % nsq, hi * h % nsq, hn * H % nsq
        return cs, rs, rns

    class Lazy(dict):
        def __missing__(self, nb):
            self[nb] = make(nb)
            return self[nb]
    return Lazy()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("nb", NBS)
def test_ragged_counts_given_r(ctxs, keys, pools, nb, count):
    N = _native()
    key = keys[nb]
    cs, rs, rns = pools[nb]
    want = [cs[i] * rns[i] % key.nsquare for i in range(count)]     # c * pow(r, n, n^2) % n^2
    ctx = ctxs.get(nb, "holder")
    ct = N.ints_to_words(cs[:count], ctx.ct_words)
    keep = ct.copy()
    out = ctx.obfuscate(ct, obf_mode=N.PAI_OBF_GIVEN, r=rs[:count])
    assert out is not ct and np.array_equal(ct, keep)
    assert N.words_to_ints(out) == want
    same = ctx.obfuscate(ct, obf_mode=N.PAI_OBF_GIVEN, r=rs[:count], out=ct)
    assert same is ct and N.words_to_ints(ct) == want


# ---------------------------------------------------------------- 3. the bits contract under device RNG
#  route            context          rows_max  crt4_min  count   kernels of r^n
ROUTES = {
    "holder_sampler": ("holder_sampler", None, None, 65),    # fixed-base sampler
    "holder_rows": ("holder", None, None, 65),               # k_crt_w
    "holder_lane": ("holder", 0, 0, 300),                    # lane CRT; k_crt4_* at 4096 bits
    "public_rows": ("public", None, None, 65),               # k_pe_w
    "public_chain": ("public", 0, None, 300),                # k_pe1_* / k_pe_* / k_pe4_*
    "public_sampler": ("public_sampler", None, None, 65),    # public fixed-base sampler
}


def _route_cases():
    for route in ROUTES:
        for nb in NBS:
            if route != "public_sampler" or nb == 2048:
                yield pytest.param(route, nb, id=f"{route}-{nb}")


@pytest.mark.parametrize("route,nb", list(_route_cases()))
def test_bits_contract_per_route(ctxs, keys, route, nb):
    N = _native()
    key = keys[nb]
    kind, rows_max, crt4_min, count = ROUTES[route]
    a, b = ctxs.get(nb, kind, 0), ctxs.get(nb, kind, 1)
    old = [(c.rows_max, c.crt4_min) for c in (a, b)]
    try:
        for c in (a, b):
            if rows_max is not None:
                c.set_rows_max(rows_max)
            if crt4_min is not None:
                c.set_crt4_min(crt4_min)
        ct, _, cs = _inputs(a, key, count, nb % 97)
        got = N.words_to_ints(a.obfuscate(ct, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE))
        e0, ex0, _ = b.encrypt(np.zeros(count, dtype=np.int64), obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE)
    finally:
        for c, (rm, cm) in zip((a, b), old):
            c.set_rows_max(rm)
            c.set_crt4_min(cm)
    E0 = N.words_to_ints(e0)
    assert not ex0.any()
    assert got == [c * e % key.nsquare for c, e in zip(cs, E0)]
    idx = _sample(count)
    if kind in ("holder", "public"):                    # the generic chains: r from the ChaCha20 stream
        rbytes = ((nb + 64 + 31) // 32) * 4
        for j, i in enumerate(idx):
            r = O.device_r(RK, BASE + i, rbytes)
            rn = pow(r, key.n, key.nsquare) if j == 0 else _powmod(r % key.nsquare, key.n, key.nsquare)
            assert got[i] == cs[i] * rn % key.nsquare, i
    elif kind == "holder_sampler":                      # O.fb_rn, with G_h = g_h^n mod h^2 computed once
        params = a.fixed_base_info()
        assert params == b.fixed_base_info()
        rb = O.fb_raw_bits(key.p, key.q)
        Gp, Gq = _powmod(params[0], key.n, key.psquare), _powmod(params[1], key.n, key.qsquare)
        inv = pow(key.qsquare, -1, key.psquare)
        for j, i in enumerate(idx):
            zp = _powmod(Gp, O.fb_exponent(RK, BASE + i, 0, key.p - 1, rb), key.psquare)
            zq = _powmod(Gq, O.fb_exponent(RK, BASE + i, 1, key.q - 1, rb), key.qsquare)
            rn = (zq + (zp - zq) * inv % key.psquare * key.qsquare) % key.nsquare
            if j == 0:
                assert rn == O.fb_rn(key, RK, BASE + i, params)
            assert got[i] == cs[i] * rn % key.nsquare, i


# ---------------------------------------------------------------- device buffers (torch)
def _dev_obfuscate(ctx, words, in_place, rng_key=RK, index_base=BASE, side_stream=False, obf_mode=None):
    """pai_obfuscate_dev on torch buffers: in place, or into a second buffer that receives r^n first."""
    import torch
    N = _native()
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    d_ct = torch.from_numpy(words.view(np.int32)).to(dev)
    d_out = d_ct if in_place else torch.empty_like(d_ct)
    stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    rc = lib.pai_obfuscate_dev(ctx.handle, d_ct.data_ptr(), words.shape[0], N.PAI_OBF_RNG if obf_mode is None else obf_mode,
                               None, 0, 0, rng_key, index_base, d_out.data_ptr(), stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    stream.synchronize()
    if not in_place:
        assert np.array_equal(d_ct.cpu().numpy().view(np.uint32), words), "the input of an out-of-place call is kept"
    return d_out.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- 4. slicing
@pytest.mark.parametrize("kind", ["holder_sampler", "holder"])
@pytest.mark.parametrize("nb", NBS)
def test_slices_do_not_change_the_bits(ctxs, keys, nb, kind):
    ctx = ctxs.get(nb, kind)
    ct, _, _ = _inputs(ctx, keys[nb], 200, 11)
    assert ctx.obf_chunk == 262144
    whole = _dev_obfuscate(ctx, ct, in_place=False)          # unsliced, r^n straight into the output
    ctx.set_obf_chunk(64)
    try:
        assert ctx.obf_chunk == 64
        sliced = _dev_obfuscate(ctx, ct, in_place=True)       # slices of 64, 64, 64 and 8
        host = ctx.obfuscate(ct, rng_key=RK, index_base=BASE, out=ct.copy())
    finally:
        ctx.set_obf_chunk(262144)
    assert np.array_equal(sliced, whole) and np.array_equal(host, whole)
    with pytest.raises(_native().NativeError):
        ctx.set_obf_chunk(63)


@pytest.mark.parametrize("nb", NBS)
def test_two_calls_on_the_halves_equal_one_call(ctxs, keys, nb):
    ctx = ctxs.get(nb, "holder")
    ct, _, _ = _inputs(ctx, keys[nb], 200, 12)
    whole = ctx.obfuscate(ct, rng_key=RK, index_base=0)
    lo = ctx.obfuscate(ct[:100], rng_key=RK, index_base=0)
    hi = ctx.obfuscate(ct[100:], rng_key=RK, index_base=100)
    assert np.array_equal(np.concatenate([lo, hi]), whole)


# ---------------------------------------------------------------- 5. semantics
@pytest.mark.parametrize("nb", NBS)
def test_semantics(ctxs, keys, nb):
    ctx = ctxs.get(nb, "holder_sampler")
    ct, ex, _ = _inputs(ctx, keys[nb], 40, 13)
    k1, k2 = hashlib.sha256(b"obf-1").digest(), hashlib.sha256(b"obf-2").digest()
    o1 = ctx.obfuscate(ct, rng_key=k1)
    o2 = ctx.obfuscate(ct, rng_key=k2)
    assert (o1 != ct).any(axis=1).all(), "every output differs from its input"
    assert (o1 != o2).any(axis=1).all(), "two rng keys give different outputs"
    v0, m0, s0, r0 = ctx.decrypt(ct, ex, want_raw=True)
    for o in (o1, o2):
        v, m, s, r = ctx.decrypt(o, ex, want_raw=True)
        assert np.array_equal(v, v0) and np.array_equal(s, s0) and np.array_equal(r, r0)
    # the inputs themselves: a float64 keeps at least 50 of its 53 bits through the base-16 encoder (4 e <= 53 - fe)
    assert np.allclose(v0, _mixed(40, 13), rtol=2.0 ** -49, atol=0.0)


# ---------------------------------------------------------------- 6. the device entry point
def test_device_entry_on_a_side_stream(ctxs, keys):
    import torch
    N = _native()
    ctx = ctxs.get(2048, "holder")
    ct, _, _ = _inputs(ctx, keys[2048], 150, 14)
    got = _dev_obfuscate(ctx, ct, in_place=True, side_stream=True)
    assert np.array_equal(got, ctx.obfuscate(ct, rng_key=RK, index_base=BASE))
    lib, W = ctx.lib, ctx.ct_words
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.zeros((20, W), dtype=torch.int32, device=dev)
    out = torch.zeros((10, W), dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    assert lib.pai_obfuscate_dev(ctx.handle, p, 10, N.PAI_OBF_NONE, None, 0, 0, RK, 0, out.data_ptr(), s) == -1
    assert lib.pai_obfuscate_dev(ctx.handle, p, 10, N.PAI_OBF_RNG, None, 0, 0, RK, 0, p + 5 * W * 4, s) == -1   # overlap
    assert lib.pai_obfuscate_dev(ctx.handle, p + 5 * W * 4, 10, N.PAI_OBF_RNG, None, 0, 0, RK, 0, p, s) == -1
    assert lib.pai_obfuscate_dev(ctx.handle, p, 10, N.PAI_OBF_RNG, None, 0, 0, None, 0, out.data_ptr(), s) == -1  # no key
    assert lib.pai_obfuscate_dev(ctx.handle, p, 10, N.PAI_OBF_GIVEN, None, 0, 0, RK, 0, out.data_ptr(), s) == -1  # no r
    assert lib.pai_obfuscate_dev(ctx.handle, p, 10, N.PAI_OBF_RNG, None, 0, 0, RK, 0, p + 10 * W * 4, s) == 0  # adjacent
    torch.cuda.synchronize()
    host = np.zeros((4, W), dtype=np.uint32)
    assert lib.pai_obfuscate(ctx.handle, host.ctypes.data, 4, N.PAI_OBF_NONE, None, 0, 0, RK, 0, host.ctypes.data) == -1
    assert lib.pai_obfuscate(ctx.handle, host.ctypes.data, 4, N.PAI_OBF_RNG, None, 0, 0, None, 0, host.ctypes.data) == -1


# ---------------------------------------------------------------- 7. the package
@pytest.fixture(scope="module")
def pkg():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    pk, sk = generate_paillier_keypair(1024, seed=7)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    a = np.random.default_rng(1).standard_normal(50)
    b = np.random.default_rng(2).standard_normal(50) * 100.0
    return pk, enc, dec, _runtime.context(pk), a, b


def _cts(arr):
    return [e.ciphertext(False) for e in np.asarray(arr).reshape(-1)]


def _flags(arr):
    return [e._is_obfuscated() for e in np.asarray(arr).reshape(-1)]


def test_array_apply_obfuscation(pkg):
    pk, enc, dec, ctx, a, b = pkg
    s = enc.encrypt(a) + enc.encrypt(b)
    assert not any(_flags(s))
    elems, before, want = list(s), _cts(s), dec.decrypt(s)
    c0 = dict(ctx.calls)
    assert s.apply_obfuscation() is s
    assert ctx.calls["pai_obfuscate"] - c0.get("pai_obfuscate", 0) == 1
    assert all(x is y for x, y in zip(list(s), elems)), "the same element objects"
    assert all(_flags(s))
    assert all(x != y for x, y in zip(_cts(s), before))
    assert s._valid_packed() is not None
    assert np.array_equal(dec.decrypt(s), want) and np.allclose(want, a + b, rtol=1e-12, atol=1e-12)
    c1 = dict(ctx.calls)
    after = _cts(s)
    s.apply_obfuscation()
    assert ctx.calls["pai_obfuscate"] == c1["pai_obfuscate"], "a second call makes no GPU call"
    assert [e.ciphertext() for e in s] == after, "ciphertext(be_secure=True) has nothing left to do"
    assert ctx.calls["pai_encrypt"] == c1.get("pai_encrypt", 0)
    # the re-randomised ciphertexts are what the packed cache feeds the next GPU operator
    assert np.array_equal(dec.decrypt(s + s), dec.decrypt(s) * 2)


def test_mixed_array_rerandomises_only_the_unflagged(pkg):
    from flex.crypto.paillier.cipher_array import PaillierArray
    pk, enc, dec, ctx, a, b = pkg
    fresh = enc.encrypt(a[:20])
    s = enc.encrypt(a[20:]) + enc.encrypt(b[20:])
    assert all(_flags(fresh)) and not any(_flags(s))
    mixed = PaillierArray(np.concatenate([np.asarray(fresh), np.asarray(s)]))
    before = _cts(mixed)
    c0 = dict(ctx.calls)
    mixed.apply_obfuscation()
    assert ctx.calls["pai_obfuscate"] - c0.get("pai_obfuscate", 0) == 1
    after = _cts(mixed)
    assert after[:20] == before[:20], "the flagged half is bit-identical"
    assert all(x != y for x, y in zip(after[20:], before[20:]))
    assert all(_flags(mixed)) and mixed._valid_packed() is not None
    assert np.allclose(dec.decrypt(mixed), np.concatenate([a[:20], a[20:] + b[20:]]), rtol=1e-12, atol=1e-12)


def test_buffer_apply_obfuscation_builds_no_objects(pkg, monkeypatch):
    from flex.crypto.paillier.cipher_array import from_wire
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    pk, enc, dec, ctx, a, b = pkg
    buf = enc.encrypt_to_buffer(a) + enc.encrypt_to_buffer(b)
    assert not buf.obfuscated.any()
    plain_wire = buf.to_wire()

    def boom(*args, **kw):
        raise AssertionError("a PaillierEncryptedNumber was built on the object-free path")
    monkeypatch.setattr(PaillierEncryptedNumber, "_make", classmethod(boom))
    monkeypatch.setattr(PaillierEncryptedNumber, "__init__", boom)
    monkeypatch.setattr("flex.crypto.paillier.cipher_array._make_numbers", boom)
    words = buf.words.copy()
    c0 = dict(ctx.calls)
    assert buf.to_wire() == plain_wire, "the default to_wire ships today's bytes"
    wire = buf.to_wire(be_secure=True)
    assert ctx.calls["pai_obfuscate"] - c0.get("pai_obfuscate", 0) == 1
    assert buf.obfuscated.all() and (buf.words != words).any(axis=1).all()
    assert buf.apply_obfuscation() is buf and ctx.calls["pai_obfuscate"] - c0.get("pai_obfuscate", 0) == 1
    back = from_wire(wire, pk, lazy=True)
    assert back.obfuscated.all() and np.array_equal(back.words, buf.words)
    monkeypatch.undo()
    assert np.allclose(dec.decrypt(back), a + b, rtol=1e-12, atol=1e-12)


def test_to_wire_be_secure(pkg):
    from flex.crypto.paillier.cipher_array import from_wire, to_wire
    pk, enc, dec, ctx, a, b = pkg
    s = enc.encrypt(a) + enc.encrypt(b)
    plain = to_wire(s)
    assert plain == to_wire(s, be_secure=False) and not from_wire(plain, pk, lazy=True).obfuscated.any()
    secure = to_wire(s, be_secure=True)
    back = from_wire(secure, pk)
    assert all(_flags(back)) and all(_flags(s)) and _cts(back) == _cts(s)
    assert from_wire(secure, pk, lazy=True).obfuscated.all()
    assert np.array_equal(dec.decrypt(back), dec.decrypt(from_wire(plain, pk)))


def test_apply_obfuscation_array_random_value(pkg):
    from flex.crypto.paillier.obfuscator import apply_obfuscation, apply_obfuscation_array
    N = _native()
    pk, enc, dec, ctx, a, b = pkg
    s = enc.encrypt(a[:6]) + enc.encrypt(b[:6])
    words = N.ints_to_words(_cts(s), ctx.ct_words)
    one = apply_obfuscation_array(words, pk, 1)
    assert one is not words and np.array_equal(one, words)
    r = pk.nsquare + 12345                                        # reduced mod n^2, as _encrypt_numpy reduces it
    got = N.words_to_ints(apply_obfuscation_array(words, pk, r))
    assert got == [c * pow(12345, pk.n, pk.nsquare) % pk.nsquare for c in _cts(s)]
    assert got[0] == apply_obfuscation(_cts(s)[0], pk, r)
