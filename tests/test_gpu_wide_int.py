"""Wide integers (PAI_BIG: Python ints beyond 64 bits) on the device -- pai_encrypt_big, pai_mul_big, pai_add_plain_big
(k_big_c0, k_mul_big) and the Python operators over them -- against Python integer arithmetic (pow, %, the key's
fields), bit-exact, at the seeded golden keys of 1024 and 2048 bits (groups of 2 and 4 lanes) and, for mul, 4096 bits
(8 lanes)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LANE_BITS = 28 * 37                                  # bn_group.hpp: LB * L, the bits of one lane's limbs


def _N():
    from flex.crypto.paillier import _native
    return _native


@pytest.fixture(scope="module")
def keys(golden):
    """bits -> (public-only context, public key, private key), made on first use."""
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    made = {}

    def get(bits):
        if bits not in made:
            k = golden["keys"][str(bits)]
            pk = PaillierPublicKey(int(k["n"], 16))
            made[bits] = (_N().Context(pk.n, 0), pk, PaillierPrivateKey(pk, int(k["p"], 16), int(k["q"], 16)))
        return made[bits]
    return get


def _rand_below(rng, bound, count):
    nbytes = (bound.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rng.bytes(nbytes), "little") % bound for _ in range(count)]


def _obj(vals):
    a = np.empty(len(vals), dtype=object)
    a[:] = vals
    return a


@pytest.mark.parametrize("bits", [1024, 2048])
def test_encrypt(keys, bits):
    N = _N()
    ctx, pk, _ = keys(bits)
    n, nsq, mx = pk.n, pk.nsquare, pk.max_int
    rng = np.random.default_rng(bits)
    vals = [0, 1, -1, 2**63 - 1, -(2**63 - 1), 2**63, 2**64, -2**64, 2**84 - 1, 2**84,
            2**LANE_BITS - 1, 2**LANE_BITS,          # the top limb is a lane's last limb; the next lane's first
            mx, -mx, mx + 1, n - 1]
    # fillers up to 67 elements: random widths from one limb to nb - 3 bits, both signs, short next to full-width
    for w in rng.integers(1, bits - 2, 67 - len(vals)).tolist():
        vals.append((_rand_below(rng, 1 << w, 1)[0] | 1 << (w - 1)) * (-1 if w & 1 else 1))
    rs = _rand_below(rng, n, len(vals))
    x, neg, wide = N.big_operand(_obj(vals), ctx.ct_words)
    # (at 1024 bits the two lane-boundary values are wider than any plaintext of the key: sent as 0 and flagged here)
    assert (wide is None) == (bits == 2048) and x.shape[1] == (bits + 31) // 32
    ct, ex, st = ctx.encrypt_big(x, neg, N.PAI_OBF_GIVEN, r=rs)
    st = st if wide is None else np.where(wide, N.EL_ENC_RANGE, st)
    got = N.words_to_ints(ct)
    for i, (v, r) in enumerate(zip(vals, rs)):
        if abs(v) > mx:
            assert st[i] == N.EL_ENC_RANGE, (i, v)
        else:
            assert st[i] == N.EL_OK and ex[i] == 0 and got[i] == (1 + n * (v % n)) * pow(r, n, nsq) % nsq, (i, v)
    assert len(vals) == 67 and np.flatnonzero(st).tolist() == ([10, 11] if bits == 1024 else []) + [14, 15]
    # below 2^63: the bits of the int64 call
    small = [i for i, v in enumerate(vals) if abs(v) < 2**63]
    c64, e64, _ = ctx.encrypt(np.array([vals[i] for i in small], dtype=np.int64), obf_mode=N.PAI_OBF_GIVEN,
                              r=[rs[i] for i in small])
    assert len(small) >= 5 and np.array_equal(c64, ct[small]) and np.array_equal(e64, ex[small])
    # the public interface raises the reference's ValueError for the element out of range
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    for bad in (mx + 1, n - 1):
        with pytest.raises(ValueError, match="Integer needs to be within"):
            PaillierEncryptor(pk).encrypt(_obj([2**70, bad, -5]))


@pytest.mark.parametrize("bits", [1024, 2048, 4096])
def test_mul(keys, bits):
    N = _N()
    ctx, pk, _ = keys(bits)
    nsq, mx = pk.nsquare, pk.max_int
    rng = np.random.default_rng(bits + 1)
    # 1 bit, 63, 64, 65 and 128 bits, nb - 3 bits, max_int: the wave's window count is the full-length ladder's
    ks = [1, 2**62 + 1, 2**63 + 5, -(2**64 + 3), 2**127 + 9, -(2**(bits - 4) + 77), mx, -3]
    if bits != 4096:
        ks.append(mx + 1)                            # does not encode: status, factor 1
    cts = _rand_below(rng, nsq, len(ks))
    words = N.ints_to_words(cts, ctx.ct_words)
    exps = np.arange(-3, len(ks) - 3, dtype=np.int32)
    out, oe, st = ctx.mul(words, exps, _obj(ks))
    got = N.words_to_ints(out)
    for i, (c, k) in enumerate(zip(cts, ks)):
        assert (st[i], oe[i]) == ((N.EL_ENC_RANGE if abs(k) > mx else N.EL_OK), exps[i]), (i, k)
        assert got[i] == (1 if abs(k) > mx else pow(c, k, nsq)), (i, k)
    o64, _, _ = ctx.mul(words[1:2], exps[1:2], np.array([ks[1]], dtype=np.int64))      # 63 bits: pai_mul's bits
    assert np.array_equal(o64[0], out[1])
    for k in (2**127 + 9, -mx, 2**62 + 1):           # one scalar for all elements
        out, oe, st = ctx.mul(words[:5], exps[:5], _obj([k]))
        assert not st.any() and np.array_equal(oe, exps[:5])
        assert N.words_to_ints(out) == [pow(c, k, nsq) for c in cts[:5]], k


@pytest.mark.parametrize("bits", [1024, 2048])
def test_add_plain(keys, bits):
    """Against the package's scalar classes: PaillierEncryptedNumber.__add__ (FixedPointNumber.encode with
    max_exponent = e_x, raw encryption with r = 1, alignment)."""
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    N = _N()
    ctx, pk, _ = keys(bits)
    mx = pk.max_int
    rng = np.random.default_rng(bits + 2)
    cases = []                                       # (ciphertext exponent, value)
    for e in (0, 13, -5):
        sh = 4 * max(e, 0)
        fill = 2**(bits - 4 - sh) + 5                # nb - 3 bits after the shift
        cases += [(e, 2**100 + 1), (e, -(2**100 + 1)), (e, fill), (e, -fill), (e, 7), (e, 0),
                  (e, mx), (e, -mx), (e, mx + 1),    # at e = 13 max_int fits only before the shift
                  (e, mx >> sh), (e, (mx >> sh) + 1)]
    cts = _rand_below(rng, pk.nsquare, len(cases))
    words = N.ints_to_words(cts, ctx.ct_words)
    exps = np.array([e for e, _ in cases], dtype=np.int32)
    out, oe, st = ctx.add_plain(words, exps, _obj([v for _, v in cases]))
    got = N.words_to_ints(out)
    flagged = 0
    for i, (c, (e, v)) in enumerate(zip(cts, cases)):
        try:
            want = PaillierEncryptedNumber(pk, c, e) + v
        except ValueError:
            assert st[i] == N.EL_ENC_RANGE, (i, e, v)
            flagged += 1
            continue
        assert st[i] == N.EL_OK and (got[i], oe[i]) == (want.ciphertext(False), want.exponent), (i, e, v)
    assert flagged == 2 + 4 + 2                      # max_int + 1 twice per exponent; at 13 also +-max_int
    v = -(2**200 + 3)                                # one scalar for all elements
    out, oe, st = ctx.add_plain(words[:7], exps[:7], _obj([v]))
    want = [PaillierEncryptedNumber(pk, c, int(e)) + v for c, e in zip(cts[:7], exps[:7])]
    assert not st.any() and N.words_to_ints(out) == [w.ciphertext(False) for w in want]
    assert oe.tolist() == [w.exponent for w in want]


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("kind", ["device", "host", "array"])
def test_round_trip(keys, bits, kind):
    """encrypt -> * wide -> + wide -> - wide -> decrypt through the public classes equals the plain-integer result; on
    the device buffer only the operands, the statuses and the decrypted values cross PCIe."""
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    N = _N()
    _, pk, priv = keys(bits)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, priv)
    vals = _obj([2**100 + 3, -(2**90), 5, -(2**70 + 1), 0, 2**64])
    r = -(2**130 + 7)
    pad = _obj([2**300 + i for i in range(5)] + [-(2**310)])
    sub = 2**65
    want = vals * r + pad - sub
    W = (2 * bits + 31) // 32
    if kind == "array":
        got = dec.decrypt(enc.encrypt(vals) * r + pad - sub)
    else:
        buf = enc.encrypt_to_buffer(vals, device=kind == "device")
        up0, down0 = N.dev_io_stats()
        out = buf * r + pad - sub
        up1, down1 = N.dev_io_stats()
        if kind == "device":
            assert up1 - up0 < vals.size * W * 4 and down1 - down0 < vals.size * W * 4      # no ciphertext moved
        got = dec.decrypt(out)
    assert got.dtype == object and got.tolist() == want.tolist()
    assert (sub - enc.encrypt(vals)).shape == (6,) and dec.decrypt(sub - enc.encrypt(vals)).tolist() == (sub - vals).tolist()


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("mode", ["none", "one_r", "pool"])
def test_encrypt_other_obfuscators(keys, bits, mode):
    """The modes test_encrypt leaves, through PaillierEncryptor: no obfuscator (r = 1), one r for all elements (stride
    0), and obfuscators taken from the pool (array and device buffer; checked by decryption and the pool's count)."""
    from flex.crypto.paillier import obfuscator_pool
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    _, pk, priv = keys(bits)
    n, nsq = pk.n, pk.nsquare
    enc = PaillierEncryptor(pk)
    vals = _obj([2**100 + 3, -(2**90), 5, -pk.max_int, 0, 2**64, pk.max_int])
    if mode != "pool":
        r = 0 if mode == "none" else _rand_below(np.random.default_rng(bits + 3), n, 1)[0]
        arr = enc.encrypt(vals, random_value=r)
        assert [e.ciphertext(False) for e in arr] == [(1 + n * (v % n)) * pow(r or 1, n, nsq) % nsq for v in vals.tolist()]
        assert [e.exponent for e in arr] == [0] * vals.size
        return
    dec = PaillierDecryptor(pk, priv)
    try:
        assert enc.prepare_obfuscators(20) == 20
        for out in (enc.encrypt(vals), enc.encrypt_to_buffer(vals, device=True)):
            assert dec.decrypt(out).tolist() == vals.tolist()
        assert enc.obfuscators_ready() == 20 - 2 * vals.size
    finally:
        obfuscator_pool.drop(pk)


@pytest.mark.parametrize("odd", [np.uint64(5), np.int8(1)], ids=["uint64", "int8"])
def test_other_numpy_integers_keep_the_type_error(keys, odd):
    """Integers that FixedPointNumber.encode refuses stay on the per-element path and raise its TypeError."""
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    enc = PaillierEncryptor(keys(1024)[1])
    vals = _obj([odd, 2**70])
    arr = enc.encrypt(_obj([2**70, 3]))
    buf = CiphertextBuffer.from_array(arr)
    for call in (lambda: enc.encrypt(vals), lambda: enc.encrypt_to_buffer(vals), lambda: arr * vals, lambda: arr + vals,
                 lambda: buf * vals, lambda: buf + vals):
        with pytest.raises(TypeError):
            call()
