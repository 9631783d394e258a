"""Packed plaintexts on the GPU: pai_encrypt_packed[_dev] / pai_decrypt_packed[_dev] (csrc/kernels_pack.hpp: k_pack_mul
over the r^n of the encrypt chains, k_unpack behind the decrypt chains) and the package layer (packed_buffer.py).

Expectations are Python integers: the pack / unpack definitions of include/flexpai.h restated in a few lines below, the
CPU oracle, and the reference's own ciphertexts (tests/golden/paillier_golden_packed.json).

* c0 = 1 + n (M mod n) exactly, without an obfuscator, over layouts, counts around a block's groups and value patterns;
* the reference fixture bit for bit under explicit r, and its sums and products through pai_add / pai_mul;
* the bits contract under device RNG on every encrypt route: ct = c0 * E0 mod n^2 with E0 the encryption of int64 zeros
  on an identically prepared second context (no pow at all);
* ragged counts, round trips against integers, statuses, the device entry points, the package in an HE_SA_FT shape.
"""
import json
import math
import os

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (1024, 2048, 4096)
RK = bytes(range(60, 92))
BASE = 11
I64_MAX = (1 << 63) - 1


def _native():
    from flex.crypto.paillier import _native
    return _native


# ---------------------------------------------------------------- the contract, in Python integers
def pack(ts, sb):
    return sum(int(t) << (sb * j) for j, t in enumerate(ts))


def unpack(m, n, sb, k):
    """The k signed digits of the raw plaintext m, or None where the contract says PAI_EL_OVERFLOW."""
    max_int = n // 3 - 1
    if m <= max_int:
        M = m
    elif m >= n - max_int:
        M = m - n
    else:
        return None
    B, out = 1 << sb, []
    for _ in range(k):
        t = ((M + B // 2) % B) - B // 2
        out.append(t)
        M = (M - t) // B
    return out if M == 0 else None


def encode(v, e, vb):
    """t of one input value at exponent e, or None where the contract says PAI_EL_ENC_RANGE."""
    if isinstance(v, (float, np.floating)):
        v = float(v)
        if math.isnan(v) or math.isinf(v):
            return None
        t = 0 if abs(v) < 1e-200 else round(math.ldexp(v, 4 * e))     # round(): ties to even, like rint
    else:
        t = int(v) << (4 * e) if e >= 0 else round(math.ldexp(float(int(v)), 4 * e))
    return t if abs(t) <= (1 << (vb - 1)) - 1 else None


def expected_c0(x, lay, n):
    """(c0 per ciphertext, statuses, slot integers) of the values x under lay = (sb, vb, e, k)."""
    sb, vb, e, k = lay
    ts = [encode(v, e, vb) for v in x]
    st = [5 if t is None else 0 for t in ts]
    ts = [0 if t is None else t for t in ts]
    C = -(-len(ts) // k)
    c0 = [(1 + n * (pack(ts[c * k:(c + 1) * k], sb) % n)) % (n * n) for c in range(C)]
    return c0, st, ts


def values_from_t(ts, dtype, e):
    """Inputs of `dtype` that encode to the integers ts at exponent e (the caller keeps them representable)."""
    if dtype == np.int64:
        assert all(t % (1 << (4 * e)) == 0 for t in ts)
        return np.array([t >> (4 * e) for t in ts], dtype=np.int64)
    x = np.array([math.ldexp(float(t), -4 * e) for t in ts], dtype=dtype)
    assert all(round(math.ldexp(float(v), 4 * e)) == t for v, t in zip(x, ts))
    return x


@pytest.fixture(scope="module")
def golden_packed():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_packed.json")) as f:
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


@pytest.fixture(scope="module")
def ctxs(keys, pfb_bases):
    from test_gpu_obfuscate import _Ctxs
    return _Ctxs(keys, pfb_bases)


def _patterns(C, k, vb, step, seed):
    """C ciphertexts' slot integers, the six patterns in turn; every integer is a multiple of `step`."""
    mx = ((1 << (vb - 1)) - 1) // step * step
    rng = np.random.default_rng(seed)
    rows = []
    for c in range(C):
        kind = c % 6
        if kind == 0:
            row = [mx] * k
        elif kind == 1:
            row = [-mx] * k                       # M < 0: a borrow runs through every slot
        elif kind == 2:
            row = [mx if j % 2 == 0 else -mx for j in range(k)]
        elif kind == 3:
            row = [0] * k                         # c0 = 1
        elif kind == 4:
            row = [0] * (k - 1) + [-mx if c % 12 == 4 else mx]
        else:
            row = [int(rng.integers(-(mx // step), mx // step + 1)) * step if mx < (1 << 62)
                   else int.from_bytes(rng.bytes(8), "little", signed=True) % mx for _ in range(k)]
        rows += row
    return rows


# ---------------------------------------------------------------- 1. c0 exact (no obfuscator, no pow)
C0_LAYOUTS = [
    pytest.param(16, 16, 3, np.float32, id="16-16-f32"),
    pytest.param(24, 20, 2, np.float32, id="24-20-f32"),
    pytest.param(40, 33, 6, np.float64, id="40-33-f64"),
    pytest.param(40, 33, 2, np.int64, id="40-33-i64-e2"),
    pytest.param(56, 56, 0, np.int64, id="56-56-i64"),
    pytest.param(64, 64, 0, np.int64, id="64-64-i64"),
]


@pytest.mark.parametrize("sb,vb,e,dtype", C0_LAYOUTS)
@pytest.mark.parametrize("nb", NBS)
def test_c0_exact(ctxs, keys, nb, sb, vb, e, dtype):
    N = _native()
    key = keys[nb]
    ctx = ctxs.get(nb, "public")
    k = ctx.pack_max_slots(sb)
    assert k == (nb - 2) // sb
    lay = (sb, vb, e, k)
    step = 1 << (4 * e) if dtype == np.int64 else 1
    for C in (1, 63, 64, 65, 129):        # around a block's 64 groups at TPI 4, and its 128 at TPI 2
        ts = _patterns(C, k, vb, step, nb + sb + C)
        x = values_from_t(ts, dtype, e)
        if dtype != np.int64:
            zeros = np.flatnonzero(x == 0)
            x[zeros[::2]] = -0.0
            assert C < 4 or np.signbit(x[zeros[0]])
        want, st_want, _ = expected_c0(x, lay, key.n)
        assert not any(st_want)
        ct, st = ctx.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_NONE)
        assert not st.any()
        got = N.words_to_ints(ct)
        assert got == want, [i for i in range(C) if got[i] != want[i]][:8]
        if C >= 4:
            assert got[3] == 1


# ---------------------------------------------------------------- 2. the reference fixture, explicit r
@pytest.mark.parametrize("party", ["holder", "public"])
@pytest.mark.parametrize("nb", NBS)
def test_reference_fixture(ctxs, keys, golden_packed, nb, party):
    N = _native()
    key = keys[nb]
    ctx = ctxs.get(nb, party)
    for rec in golden_packed["cases"][str(nb)]:
        lay = (rec["slot_bits"], rec["value_bits"], rec["exponent"], rec["slots"])
        k = lay[3]
        ts = [t for row in rec["t"] for t in row]
        x = values_from_t(ts, np.float64, lay[2])
        ct, st = ctx.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_GIVEN, r=[int(r, 16) for r in rec["r"]])
        assert not st.any()
        assert [hex(c) for c in N.words_to_ints(ct)] == rec["ct"]
        if party != "holder":
            continue
        ex = np.full(1, lay[2], dtype=np.int32)
        s3, e3 = ctx.add([ct[0:1], ct[1:2], ct[2:3]], [ex, ex, ex])
        m3, em, _ = ctx.mul(ct[0:1], ex, np.array([-3], dtype=np.int64))
        assert hex(N.words_to_ints(s3)[0]) == rec["sum3"] and hex(N.words_to_ints(m3)[0]) == rec["mul_m3"]
        assert int(e3[0]) == lay[2] and int(em[0]) == lay[2]
        val, mant, st = ctx.decrypt_packed(np.concatenate([ct, s3, m3]), lay, 5 * k)
        assert not st.any()
        rows = rec["t"] + [[a + b + c for a, b, c in zip(*rec["t"])], [-3 * a for a in rec["t"][0]]]
        assert mant.tolist() == [t for row in rows for t in row]
        raws = [int(h, 16) for h in rec["raw"] + [rec["raw_sum3"], rec["raw_mul_m3"]]]
        assert [unpack(m, key.n, lay[0], k) for m in raws] == rows


# ---------------------------------------------------------------- 3. the bits contract under device RNG
def _route_cases():
    from test_gpu_obfuscate import ROUTES
    for route in ROUTES:
        for nb in NBS:
            if route != "public_sampler" or nb == 2048:
                yield pytest.param(route, nb, id=f"{route}-{nb}")


@pytest.mark.parametrize("route,nb", list(_route_cases()))
def test_bits_contract_per_route(ctxs, keys, route, nb):
    from test_gpu_obfuscate import ROUTES
    N = _native()
    key = keys[nb]
    kind, rows_max, crt4_min, count = ROUTES[route]
    a, b = ctxs.get(nb, kind, 0), ctxs.get(nb, kind, 1)
    sb, vb, e = 32, 24, 5
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    nvals = count * k - 3
    x = values_from_t(_patterns(count, k, vb, 1, nb)[:nvals], np.float32, e)
    old = [(c.rows_max, c.crt4_min) for c in (a, b)]
    try:
        for c in (a, b):
            if rows_max is not None:
                c.set_rows_max(rows_max)
            if crt4_min is not None:
                c.set_crt4_min(crt4_min)
        ct, st = a.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE)
        e0, ex0, _ = b.encrypt(np.zeros(count, dtype=np.int64), obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE)
        h = count // 2
        lo, _ = a.encrypt_packed(x[:h * k], lay, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE)
        hi, _ = a.encrypt_packed(x[h * k:], lay, obf_mode=N.PAI_OBF_RNG, rng_key=RK, index_base=BASE + h)
    finally:
        for c, (rm, cm) in zip((a, b), old):
            c.set_rows_max(rm)
            c.set_crt4_min(cm)
    assert not st.any() and not ex0.any()
    c0, _, _ = expected_c0(x, lay, key.n)
    E0 = N.words_to_ints(e0)
    assert len(set(E0)) == count and 1 not in E0
    assert N.words_to_ints(ct) == [c * s % key.nsquare for c, s in zip(c0, E0)]
    assert np.array_equal(np.concatenate([lo, hi]), ct), "index_base counts ciphertexts"


# ---------------------------------------------------------------- 4. ragged N
@pytest.mark.parametrize("nb", NBS)
def test_ragged_counts(ctxs, keys, nb):
    N = _native()
    key = keys[nb]
    ctx = ctxs.get(nb, "holder")
    sb, vb, e = 24, 24, 0
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    ts = _patterns(4, k, vb, 1, nb + 1)
    ts = [t if t else 5 for t in ts]                      # no zeros: a top slot left zero is the call's doing
    for n in (1, k - 1, k, k + 1, 3 * k + 2):
        x = np.array(ts[:n], dtype=np.int64)
        want, _, _ = expected_c0(x, lay, key.n)
        ct, st = ctx.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_NONE)
        assert ct.shape == (-(-n // k), ctx.ct_words) and st.shape == (n,) and not st.any()
        assert N.words_to_ints(ct) == want
        last = unpack((want[-1] - 1) // key.n, key.n, sb, k)
        assert last[(n - 1) % k + 1:] == [0] * (k - 1 - (n - 1) % k) and last[(n - 1) % k] == ts[n - 1]
        val, mant, st = ctx.decrypt_packed(ct, lay, n)
        assert mant.tolist() == ts[:n] and not st.any() and val.tolist() == [float(t) for t in ts[:n]]


# ---------------------------------------------------------------- 5. round trips against integers
@pytest.mark.parametrize("nb", NBS)
def test_round_trips(ctxs, keys, nb):
    N = _native()
    ctx = ctxs.get(nb, "holder")
    rng = np.random.default_rng(nb + 5)
    # fresh ciphertexts under device RNG, float64 at e = 10
    sb, vb, e = 64, 53, 10
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    mx = (1 << (vb - 1)) - 1
    n = 3 * k - 1
    ts = [int(v) for v in rng.integers(-mx, mx + 1, n)]
    ts[:3] = [mx, -mx, 0]
    ct, st = ctx.encrypt_packed(values_from_t(ts, np.float64, e), lay, rng_key=RK)
    val, mant, st2 = ctx.decrypt_packed(ct, lay, n)
    assert not st.any() and not st2.any() and mant.tolist() == ts
    assert val.tolist() == [float(t) * 16.0 ** -e for t in ts]
    # products by 3, -1 and -(2^20): every slot scales at once
    sb, vb, e = 64, 40, 3
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    mx = (1 << (vb - 1)) - 1
    ts = [int(v) for v in rng.integers(-mx, mx + 1, 2 * k)]
    ts[:2] = [mx, -mx]
    ct, _ = ctx.encrypt_packed(values_from_t(ts, np.float64, e), lay, rng_key=RK)
    ex = np.full(2, e, dtype=np.int32)
    for s in (3, -1, -(1 << 20)):
        out, oe, _ = ctx.mul(ct, ex, np.array([s], dtype=np.int64))
        assert oe.tolist() == [e, e]
        val, mant, st = ctx.decrypt_packed(out, lay, 2 * k)
        assert not st.any() and mant.tolist() == [s * t for t in ts]
        assert val.tolist() == [float(s * t) * 16.0 ** -e for t in ts]
    # an 8-way add whose slot sums reach exactly +-(2^(sb-1) - 1)
    sb, vb, e = 32, 32, 4
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    lim = (1 << (sb - 1)) - 1
    parts = [[int(v) for v in rng.integers(0, lim // 8, k)] for _ in range(7)]
    parts.insert(0, [lim - sum(col) for col in zip(*parts)])
    sign = [1 if j % 2 == 0 else -1 for j in range(k)]
    cts = [ctx.encrypt_packed(np.array([s * t for s, t in zip(sign, p)], dtype=np.float64) * 16.0 ** -e, lay,
                              rng_key=RK, index_base=i)[0] for i, p in enumerate(parts)]
    ex = np.full(1, e, dtype=np.int32)
    out, oe = ctx.add(cts, [ex] * 8)
    val, mant, st = ctx.decrypt_packed(out, lay, k)
    assert not st.any() and mant.tolist() == [s * lim for s in sign]
    assert val.tolist() == [float(s * lim) * 16.0 ** -e for s in sign]
    # (64, 64): the int64 extremes
    lay = (64, 64, 0, (nb - 2) // 64)
    x = np.array([I64_MAX, -I64_MAX, 0, -1, 1, I64_MAX - 1], dtype=np.int64)
    ct, st = ctx.encrypt_packed(x, lay, rng_key=RK)
    val, mant, st2 = ctx.decrypt_packed(ct, lay, x.size)
    assert not st.any() and not st2.any() and np.array_equal(mant, x)
    assert val.tolist() == [float(int(v)) for v in x]


# ---------------------------------------------------------------- 6. statuses
@pytest.mark.parametrize("nb", NBS)
def test_statuses(ctxs, keys, nb):
    N = _native()
    key = keys[nb]
    ctx = ctxs.get(nb, "holder")
    sb, vb, e = 32, 24, 5
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    mx = (1 << (vb - 1)) - 1
    ts = [int(v) for v in np.random.default_rng(nb).integers(-mx, mx + 1, 2 * k)]
    x = values_from_t(ts, np.float64, e)
    bad = {1: (mx + 1) * 16.0 ** -e, 4: -(mx + 1) * 16.0 ** -e, k - 1: float("nan"), k: float("inf"), k + 3: float("-inf")}
    for i, v in bad.items():
        x[i] = v
    x[2], x[k + 1] = mx * 16.0 ** -e, -mx * 16.0 ** -e          # the last values in range, next to the first ones out
    want, st_want, tz = expected_c0(x, lay, key.n)
    ct, st = ctx.encrypt_packed(x, lay, obf_mode=N.PAI_OBF_NONE)
    assert st.tolist() == st_want and sorted(np.flatnonzero(st)) == sorted(bad) and set(st[list(bad)]) == {N.EL_ENC_RANGE}
    assert N.words_to_ints(ct) == want
    val, mant, st = ctx.decrypt_packed(ct, lay, 2 * k)
    assert not st.any() and mant.tolist() == tz and all(mant[i] == 0 for i in bad)
    # decrypt: a plaintext in the gap, and M = B^k, each flag their own ciphertext's values and no other
    n, nsq = key.n, key.nsquare
    good = pack(ts[:k], sb) % n
    for m in (n // 2, 1 << (sb * k)):
        assert unpack(m, n, sb, k) is None
        cts = N.ints_to_words([(1 + n * good) % nsq, (1 + n * m) % nsq, (1 + n * good) % nsq], ctx.ct_words)
        val, mant, st = ctx.decrypt_packed(cts, lay, 3 * k - 2)
        assert st.tolist() == [0] * k + [N.EL_OVERFLOW] * k + [0] * (k - 2)
        assert mant.tolist() == ts[:k] + [0] * k + ts[:k - 2]
    # errors
    import ctypes
    lib = ctx.lib
    pub = ctxs.get(nb, "public")
    val, mant, st = (np.zeros(k), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32))
    ok = N.pack_layout(lay)
    assert lib.pai_decrypt_packed(pub.handle, cts.ctypes.data, ctypes.byref(ok), k, val.ctypes.data, mant.ctypes.data,
                                  st.ctypes.data) == -3
    with pytest.raises(N.NativeError, match="flexpai error -3"):
        pub.decrypt_packed(cts[:1], lay, k)
    xs = np.zeros(k, dtype=np.float64)
    out = np.zeros((k, ctx.ct_words), dtype=np.uint32)
    for badlay in ((20, 16, 0, 3), (32, 33, 0, 3), (32, 1, 0, 3), (32, 24, 0, k + 1), (32, 24, 0, 0), (8, 8, 0, 3),
                   (72, 64, 0, 3)):
        bl = N.pack_layout(badlay)
        for c in (ctx, pub):
            assert lib.pai_encrypt_packed(c.handle, N.PAI_F64, xs.ctypes.data, 3, ctypes.byref(bl), N.PAI_OBF_NONE, None,
                                          0, 0, RK, 0, out.ctypes.data, None) == -1, badlay
        assert lib.pai_decrypt_packed(ctx.handle, out.ctypes.data, ctypes.byref(bl), 3, val.ctypes.data,
                                      mant.ctypes.data, st.ctypes.data) == -1, badlay
    slots = ctypes.c_int()
    assert lib.pai_pack_max_slots(ctx.handle, 20, ctypes.byref(slots)) == -1


# ---------------------------------------------------------------- 7. the device entry points
def test_device_entry_on_a_side_stream(ctxs, keys):
    import ctypes
    import torch
    N = _native()
    nb = 2048
    ctx = ctxs.get(nb, "holder")
    sb, vb, e = 32, 24, 5
    k = (nb - 2) // sb
    lay = (sb, vb, e, k)
    C = 70
    nvals = C * k - 5
    x = values_from_t(_patterns(C, k, vb, 1, 7)[:nvals], np.float32, e)
    x[9] = np.float32("nan")
    ct, st = ctx.encrypt_packed(x, lay, rng_key=RK, index_base=BASE)
    val, mant, st2 = ctx.decrypt_packed(ct, lay, nvals)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_x = torch.from_numpy(x).to(dev)
    d_ct = torch.zeros((C, ctx.ct_words), dtype=torch.int32, device=dev)
    d_st = torch.full((nvals,), -1, dtype=torch.int32, device=dev)
    d_val = torch.zeros(nvals, dtype=torch.float64, device=dev)
    d_mant = torch.zeros(nvals, dtype=torch.int64, device=dev)
    d_st2 = torch.full((nvals,), -1, dtype=torch.int32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    lib, L = ctx.lib, N.pack_layout(lay)
    rc = lib.pai_encrypt_packed_dev(ctx.handle, N.PAI_F32, d_x.data_ptr(), nvals, ctypes.byref(L), N.PAI_OBF_RNG, None, 0, 0,
                                    RK, BASE, d_ct.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    rc = lib.pai_decrypt_packed_dev(ctx.handle, d_ct.data_ptr(), ctypes.byref(L), nvals, d_val.data_ptr(),
                                    d_mant.data_ptr(), d_st2.data_ptr(), stream.cuda_stream)
    assert rc == 0, lib.pai_last_error().decode()
    stream.synchronize()
    assert np.array_equal(d_ct.cpu().numpy().view(np.uint32), ct)
    assert np.array_equal(d_st.cpu().numpy(), st) and st[9] == N.EL_ENC_RANGE and st.sum() == N.EL_ENC_RANGE
    assert np.array_equal(d_val.cpu().numpy(), val) and np.array_equal(d_mant.cpu().numpy(), mant)
    assert np.array_equal(d_st2.cpu().numpy(), st2) and not st2.any()
    want = [0 if i == 9 else round(math.ldexp(float(v), 4 * e)) for i, v in enumerate(x)]
    assert mant.tolist() == want


# ---------------------------------------------------------------- 8. the package, in an HE_SA_FT shape
def test_package_he_sa_ft():
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPublicKey, generate_paillier_keypair
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, sk = generate_paillier_keypair(1024, seed=11)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, sk)
    ctx = _runtime.context(pk)
    e = 6
    lay = PackedLayout.for_sum(pk, max_abs=60.0, exponent=e, terms=2)     # 60 * 16^6 < 2^30: one bit of headroom
    assert lay.value_bits == 31 and lay.slot_bits == 32 and lay.slots == 31
    w1 = np.random.default_rng(21).uniform(-60, 60, (40, 25)).astype(np.float32)
    w2 = np.random.default_rng(22).uniform(-60, 60, (40, 25)).astype(np.float32)
    c0 = dict(ctx.calls)
    wires = [enc.encrypt_packed(w, lay).to_wire() for w in (w1, w2)]
    assert ctx.calls["pai_encrypt_packed"] - c0.get("pai_encrypt_packed", 0) == 2
    assert len(wires[0]) < 1000 * (4 * ctx.ct_words + 5) // 25
    # the coordinator: the public key only
    pub = PaillierPublicKey(pk.n)
    bufs = [PackedCiphertextBuffer.from_wire(w, pub) for w in wires]
    c1 = dict(ctx.calls)
    total = bufs[0] + bufs[1]
    assert total.bound == 2 * bufs[0].bound and not total.obfuscated
    wire = total.to_wire(be_secure=True)
    assert total.obfuscated
    for name, cnt in (("pai_add", 1), ("pai_obfuscate", 1), ("pai_encrypt_packed", 0), ("pai_mul", 0)):
        assert ctx.calls[name] - c1.get(name, 0) == cnt, name
    with pytest.raises(OverflowError):
        total + bufs[0]
    assert ctx.calls["pai_add"] - c1.get("pai_add", 0) == 1, "refused before any GPU call"
    # the parties
    back = PackedCiphertextBuffer.from_wire(wire, pk)
    c2 = dict(ctx.calls)
    got = dec.decrypt(back)
    assert ctx.calls["pai_decrypt_packed"] - c2.get("pai_decrypt_packed", 0) == 1
    t1 = np.array([round(math.ldexp(float(v), 4 * e)) for v in w1.reshape(-1)])
    t2 = np.array([round(math.ldexp(float(v), 4 * e)) for v in w2.reshape(-1)])
    assert got.shape == (40, 25) and got.dtype == np.float64
    assert np.array_equal(got.reshape(-1), (t1 + t2).astype(np.float64) * 16.0 ** -e)
    mean = got / 2
    assert np.allclose(mean, (w1.astype(np.float64) + w2) / 2, rtol=0, atol=16.0 ** -e)
    with pytest.raises(ValueError, match="index 3"):
        bad = w1.copy().reshape(-1)
        bad[3], bad[7] = 1.0e6, np.nan
        enc.encrypt_packed(bad, lay)
