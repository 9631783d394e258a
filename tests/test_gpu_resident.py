"""Device-resident ciphertext buffers on the GPU: the transfers (pai_dev_upload / pai_dev_download and their byte
counters), pai_take_dev and pai_check_below_dev at every row width, and DeviceCiphertextBuffer / the resident
PackedCiphertextBuffer against the host classes on the same inputs, bit for bit (both sides run the same kernels); the
chain's traffic contract, buffer lifetime, and the key holder's encrypt / decrypt."""
import gc
import os
import weakref

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
EMPTY = -(1 << 31)


def _native():
    from flex.crypto.paillier import _native as N
    return N


def _key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _key1035():
    """A 1035-bit modulus (ct_words 65): the K1035 of tests/test_gpu_ops_sizes.py."""
    from test_gpu_ops_sizes import _make_key
    return _make_key("K1035", None)


def _pk(key):
    from flex.crypto.paillier.keypair import PaillierPublicKey
    return PaillierPublicKey(key.n)


def residues(pk, shape, seed, exp_hi=21):
    """A CiphertextBuffer of random residues mod n^2 with exponents 0..20 and mixed flags."""
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    W = (2 * pk.n.bit_length() + 31) // 32
    words = _native().ints_to_words([int.from_bytes(rng.bytes(4 * W + 8), "little") % pk.nsquare for _ in range(N)], W)
    return CiphertextBuffer(pk, words.reshape(N, W), rng.integers(0, exp_hi, N).astype(np.int32),
                            rng.integers(0, 2, N).astype(np.uint8), shape)


@pytest.fixture(scope="module")
def pks(golden):
    return {nb: _pk(_key(golden, nb)) for nb in (1024, 2048)}


@pytest.fixture(scope="module", params=[1024, 2048])
def pk(request, pks):
    return pks[request.param]


def eq(dev, host):
    """A device buffer against the host class's result: shape, words, exponents, flags."""
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer
    assert isinstance(dev, DeviceCiphertextBuffer) and dev.shape == host.shape and dev.size == host.size
    got = dev.to_host()
    assert np.array_equal(got.exps, host.exps) and np.array_equal(got.obfuscated, host.obfuscated)
    assert np.array_equal(got.words, host.words)


# ------------------------------------------------------------------------------- transfer
@pytest.mark.parametrize("nb", [1024, 2048])
def test_round_trip_and_byte_counters(pks, nb):
    N = _native()
    pk = pks[nb]
    W = (2 * nb) // 32
    for n in (0, 1, 3, 1100):
        buf = residues(pk, (n,), 100 + n)
        up0, down0 = N.dev_io_stats()
        dev = buf.to_device()
        up1, down1 = N.dev_io_stats()
        assert (up1 - up0, down1 - down0) == (n * W * 4 + n * 4, 0) and dev.nbytes == n * W * 4 + n * 4
        back = dev.to_host()                                            # (the exponents are cached: words only)
        up2, down2 = N.dev_io_stats()
        assert (up2 - up1, down2 - down1) == (0, n * W * 4)
        assert np.array_equal(back.words, buf.words) and np.array_equal(back.exps, buf.exps)
        assert np.array_equal(back.obfuscated, buf.obfuscated) and back.shape == buf.shape
        dev.release()


def test_small_staging_slots_span_the_array(pks, xlib, monkeypatch):
    """The test build with the slot shrunk: 1100 rows of 256 bytes cross in 3 slots, the last one ragged."""
    N = _native()
    monkeypatch.setenv("FLEXPAI_RES_SLOT", "100000")
    words = residues(pks[1024], (1100,), 7).words
    assert 2 * 100000 < words.nbytes < 3 * 100000 and words.nbytes % 100000
    up0, down0 = N.dev_io_stats(xlib)
    mem = N.DeviceMem(words.nbytes, 0, lib=xlib).upload(words)
    back = mem.download(np.uint32, words.size).reshape(words.shape)
    up1, down1 = N.dev_io_stats(xlib)
    assert np.array_equal(back, words) and (up1 - up0, down1 - down0) == (words.nbytes, words.nbytes)
    part = mem.download(np.uint32, 64 * 500, offset=256 * 300).reshape(500, 64)      # 128 000 bytes: two slots
    assert np.array_equal(part, words[300:800])
    mem.free()


# ------------------------------------------------------------------------------- pai_take_dev
@pytest.fixture(scope="module")
def take_keys(golden):
    return {64: _key(golden, 1024), 65: _key1035(), 128: _key(golden, 2048), 256: _key(golden, 4096)}


@pytest.mark.parametrize("W", [64, 65, 128, 256])
def test_take_dev_every_width(take_keys, W):
    N = _native()
    key = take_keys[W]
    ctx = N.Context(key.n, 0)
    assert ctx.ct_words == W
    src = residues(_pk(key), (37,), W)
    d_ct, d_ex = N.device_upload(src.words), N.device_upload(src.exps)
    rng = np.random.default_rng(W)
    holes = rng.integers(0, 37, 90)
    holes[::3] = -1
    cases = [np.zeros(0, dtype=np.int64), np.array([36]), np.arange(36, -1, -1), rng.integers(0, 5, 1000), holes,
             np.full(3, -1)]
    for idx in cases:
        idx = idx.astype(np.int64)
        M = idx.size
        out, oe = N.DeviceMem(M * W * 4, 0), N.DeviceMem(M * 4, 0)
        ctx.take_dev(d_ct.ptr, d_ex.ptr, 37, idx, out.ptr, oe.ptr)
        got, ge = out.download(np.uint32, M * W).reshape(M, W), oe.download(np.int32, M)
        one = np.zeros(W, dtype=np.uint32)
        one[0] = 1
        want = np.where((idx >= 0)[:, None], src.words[np.maximum(idx, 0)], one[None, :])
        assert np.array_equal(got, want) and np.array_equal(ge, np.where(idx >= 0, src.exps[np.maximum(idx, 0)], EMPTY))
    # refused before any launch, the output untouched
    mark = np.full((4, W), 0xA5A5A5A5, dtype=np.uint32)
    out, oe = N.device_upload(mark), N.device_upload(np.full(4, 77, dtype=np.int32))
    for bad in ([0, 37, 1, 2], [0, 1, -2, 2]):
        with pytest.raises(N.NativeError, match="index out of range"):
            ctx.take_dev(d_ct.ptr, d_ex.ptr, 37, np.array(bad, dtype=np.int64), out.ptr, oe.ptr)
    with pytest.raises(N.NativeError, match="null pointer"):
        ctx.take_dev(d_ct.ptr, d_ex.ptr, 37, np.arange(4), None, oe.ptr)
    assert np.array_equal(out.download(np.uint32, 4 * W).reshape(4, W), mark)
    assert np.array_equal(oe.download(np.int32, 4), np.full(4, 77))
    with pytest.raises(N.NativeError, match="overlaps"):       # the output starts inside the input
        ctx.take_dev(d_ct.ptr, d_ex.ptr, 37, np.arange(4), d_ct.at(36 * W * 4), oe.ptr)
    with pytest.raises(N.NativeError, match="overlaps"):
        ctx.take_dev(d_ct.ptr, d_ex.ptr, 37, np.arange(4), out.ptr, d_ex.at(8))
    assert np.array_equal(d_ct.download(np.uint32, 37 * W).reshape(37, W), src.words)
    assert np.array_equal(d_ex.download(np.int32, 37), src.exps)
    ctx.close()


# ------------------------------------------------------------------------------- pai_check_below_dev
@pytest.mark.parametrize("W", [64, 65, 128])
def test_check_below_dev(take_keys, W):
    N = _native()
    key = take_keys[W]
    ctx = N.Context(key.n, 0)
    good = residues(_pk(key), (41,), 3 * W).words
    nsq = key.nsquare
    edge = N.ints_to_words([nsq - 1, nsq, (1 << (32 * W)) - 1, nsq + 1, nsq - (1 << 32)], W)
    d = N.device_upload(good)
    assert ctx.check_below_dev(d.ptr, 41) == -1 and ctx.check_below_dev(d.ptr, 0) == -1
    for row, ok in ((0, True), (1, False), (2, False), (3, False), (4, True)):
        for pos in (0, 20, 40):
            words = good.copy()
            words[pos] = edge[row]
            d.upload(words)
            assert ctx.check_below_dev(d.ptr, 41) == (-1 if ok else pos)
    words = good.copy()
    words[[40, 7, 23]] = edge[1], edge[2], edge[3]
    assert ctx.check_below_dev(d.upload(words).ptr, 41) == 7            # the first bad row of several
    ctx.close()


def test_from_wire_on_the_device(pks):
    from flex.crypto.paillier.cipher_array import from_wire
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    pk = pks[1024]
    buf = residues(pk, (5, 9), 21)
    wire = buf.to_wire()
    dev = from_wire(wire, pk, lazy=True, device=True)
    eq(dev, from_wire(wire, pk, lazy=True))
    assert dev.to_wire() == wire and np.array_equal(dev.exps, buf.exps)
    words = buf.words.copy()
    words[31] = _native().ints_to_words([pk.nsquare], words.shape[1])[0]
    bad = CiphertextBuffer(pk, words, buf.exps, buf.obfuscated, buf.shape).to_wire()
    errors = []
    for device in (False, True):
        with pytest.raises(ValueError) as e:
            from_wire(bad, pk, lazy=True, device=device)
        errors.append(str(e.value))
    assert errors[0] == errors[1] == "corrupted ciphertext array (ciphertext >= n^2)"
    with pytest.raises(ValueError, match="different public key"):
        from_wire(wire, pks[2048], lazy=True, device=True)


# ------------------------------------------------------------------------------- operator parity
def test_add_sub_mul_plain(pk):
    from flex.crypto.paillier.cipher_buffer import add_buffers
    a, b, c = (residues(pk, (6, 4), s) for s in (31, 32, 33))
    da, db, dc = a.to_device(), b.to_device(), c.to_device()
    eq(add_buffers([da, db]), add_buffers([a, b]))
    eq(add_buffers([da, db, dc]), add_buffers([a, b, c]))
    eq(add_buffers([da, b, dc]), add_buffers([a, b, c]))               # a host operand is uploaded for the call
    eq(da + db, a + b)
    eq(da - db, a - b)
    eq(da - b, a - b)
    eq(a - db, a - b)
    eq(a + db, a + b)
    one = a.to_array()[1, 2]
    eq(da + one, a + one)
    flat, dflat = a.reshape(24)[:4], da.reshape(24)[:4]
    scal = np.array([-1, 3, 0.5, -2.25])
    eq(dflat * scal, flat * scal)
    eq(da * -1, a * -1)
    eq(da / 4, a / 4)
    eq(da + 2.5, a + 2.5)
    eq(3 + da, a + 3)
    eq(da - 1.25, a - 1.25)
    eq(7 - da, 7 - a)
    y = np.random.default_rng(1).standard_normal(24)
    eq(da + y.reshape(6, 4), a + y.reshape(6, 4))
    with pytest.raises(ValueError, match="is not allowed"):
        da * db
    with pytest.raises(ValueError, match="differ"):
        da + db.reshape(4, 6)


def test_flagged_elements_fall_back_to_the_host_operator(pks):
    """A float that overflows at the ciphertext's exponent: the device flags it, and the whole call runs the host class's
    operator (the reference's exception where the reference raises)."""
    from flex.crypto.paillier.device_buffer import add_plain_dev
    pk = pks[1024]
    a = residues(pk, (4,), 41, exp_hi=1)
    a.exps[:] = 300
    y = np.array([1e300, 1.0, 2.0, 3.0])
    d = a.to_device()
    st = add_plain_dev(pk, d.words, d._ex, y)[2]
    assert (st == _native().EL_FLOAT_OVF).all()                        # x * 16^300 is no finite double for |x| >= 1
    try:
        want = a + y
    except Exception as e:   # noqa: BLE001 - whatever the host class raises, the device class raises too
        with pytest.raises(type(e)):
            a.to_device() + y
    else:
        eq(a.to_device() + y, want)


def test_wrong_key_and_device(pks):
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer
    a, b = residues(pks[1024], (3,), 1), residues(pks[2048], (3,), 2)
    with pytest.raises(ValueError, match="different public key"):
        a.to_device() + b.to_device()
    with pytest.raises(ValueError, match="different public key"):
        a.to_device() + b
    d = a.to_device()
    other = DeviceCiphertextBuffer.from_pointers(a.public_key, d.data_ptr(), d.exps_ptr(), 3, owner=d, device=1)
    with pytest.raises(ValueError, match="device"):
        other.cumsum()
    with pytest.raises(ValueError, match="device"):
        d + other


def test_dot_and_segment_dot(pk):
    class Csc:
        """The duck type of a sparse matrix: .tocsc() with indptr, indices, data, shape."""
        def __init__(self, dense):
            self.shape = dense.shape
            cols = [np.flatnonzero(dense[:, j]) for j in range(dense.shape[1])]
            self.indptr = np.concatenate([[0], np.cumsum([c.size for c in cols])])
            self.indices = np.concatenate(cols)
            self.data = np.concatenate([dense[c, j] for j, c in enumerate(cols)])

        def tocsc(self):
            return self

    rng = np.random.default_rng(5)
    v, m = residues(pk, (40,), 51), residues(pk, (2, 40), 52)
    x3, x17 = rng.standard_normal((40, 3)), rng.integers(-9, 10, (40, 17)).astype(np.int64)
    eq(v.to_device() @ x3, v @ x3)
    eq(v.to_device().dot(x3[:, 0]), v.dot(x3[:, 0]))
    eq(m.to_device() @ x17, m @ x17)
    sp = np.where(rng.random((40, 6)) < 0.2, rng.standard_normal((40, 6)), 0.0)
    sp[:, 4] = 0.0                                                      # an empty column: an empty segment
    eq(v.to_device() @ Csc(sp), v @ Csc(sp))
    eq(m.to_device() @ Csc(sp), m @ Csc(sp))
    idx, off = np.array([3, 3, 39, 0, 3, 17]), np.array([0, 3, 3, 6])   # a repeated index, an empty segment
    w = np.array([1.5, -2.0, 4.0, 1.0, 0.0, -0.125])
    eq(v.to_device().segment_dot(idx, off, w), v.segment_dot(idx, off, w))
    with pytest.raises(IndexError):
        v.to_device().segment_dot([40], [0, 1], [1.0])


def _hist_inputs(dtype):
    rng = np.random.default_rng(77)
    bins = rng.integers(0, 7, (300, 3)).astype(dtype)                   # ids 5, 6 >= B = 5: in no cell
    bins[:, 2] = np.minimum(bins[:, 2], 3)                              # bin 4 of feature 2 stays empty
    node = rng.integers(-1, 3, 300)                                     # -1 and 2: in no cell
    return bins, node


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_histogram(pks, dtype):
    from flex.crypto.paillier import parallel_ops
    a = residues(pks[1024], (300,), 61)
    d = a.to_device()
    bins, node = _hist_inputs(dtype)
    want, wc = a.histogram(bins, 5, node=node, n_nodes=2)
    got, gc_ = d.histogram(bins, 5, node=node, n_nodes=2)
    assert isinstance(gc_, np.ndarray) and np.array_equal(gc_, wc) and (wc == 0).any() and got.shape == (2, 3, 5)
    eq(got, want)
    got, gc_ = parallel_ops.histogram(d, bins, 5, node=node, n_nodes=2)
    eq(got, want)
    one, c1 = d.histogram(bins[:, :1], 7)
    w1, wc1 = a.histogram(bins[:, :1], 7)
    eq(one, w1)
    assert np.array_equal(c1, wc1)


def test_histogram_2048_and_sparse(pks):
    class Csr:
        def __init__(self, dense, default):
            self.shape = dense.shape
            rows = [np.flatnonzero(dense[i] != default) for i in range(dense.shape[0])]
            self.indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
            self.indices = np.concatenate(rows)
            self.data = np.concatenate([dense[i, r] for i, r in enumerate(rows)])

        def tocsr(self):
            return self

    bins, node = _hist_inputs(np.uint8)
    a = residues(pks[2048], (300,), 62)
    d = a.to_device()
    want, wc = a.histogram(bins, 5, node=node, n_nodes=2)
    got, gc_ = d.histogram(bins, 5, node=node, n_nodes=2)
    eq(got, want)
    assert np.array_equal(gc_, wc)
    default = np.array([0, 2, 9])                                      # per feature; 9 is out of range
    stored = bins.astype(np.int64)
    keep = np.random.default_rng(3).random(stored.shape) < 0.3
    dense = np.where(keep, stored, default[None, :])
    csr = Csr(dense, default[None, :])
    b = residues(pks[1024], (300,), 63, exp_hi=1)                      # uniform exponents: the dense call's bits
    want, wc = b.histogram(csr, 5, node=node, n_nodes=2, default_bin=default)
    got, gc_ = b.to_device().histogram(csr, 5, node=node, n_nodes=2, default_bin=default)
    eq(got, want)
    assert np.array_equal(gc_, wc)


def test_cumsum_sum_reshape_indexing(pks):
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.cipher_buffer import concatenate
    a = residues(pks[1024], (4, 7, 3), 71)
    d = a.to_device()
    for axis in (0, 1, 2, -1):
        for rev in (False, True):
            eq(d.cumsum(axis, rev), a.cumsum(axis, rev))
    eq(parallel_ops.cumsum(d, 1, True), a.cumsum(1, True))
    for axis in (None, 0, -1):
        eq(d.sum(axis), a.sum(axis))
    eq(d.reshape(7, 12), a.reshape(7, 12))
    eq(d.reshape((84,)), a.reshape(84))
    mask = np.random.default_rng(2).integers(0, 2, 4).astype(bool)
    for key in (2, -1, slice(1, 3), slice(None, None, -2), (Ellipsis, 0), [[0, 3, 3]], mask, slice(2, 2), (1, 6, 2)):
        eq(d[key], a[key])
    eq(d.take([6, 0, 0, -2], axis=1), a.take([6, 0, 0, -2], axis=1))
    eq(d.T, a.T)
    eq(d.transpose(1, 0, 2), a.transpose(1, 0, 2))
    b = residues(pks[1024], (2, 7, 3), 72)
    eq(concatenate([d, b.to_device(), d]), concatenate([a, b, a]))
    eq(concatenate([a, b.to_device()]), concatenate([a, b]))
    c = residues(pks[1024], (4, 7, 5), 73)
    eq(concatenate([d, c.to_device()], axis=2), concatenate([a, c], axis=2))
    # 2048 bits, one pass
    a2 = residues(pks[2048], (3, 5), 74)
    d2 = a2.to_device()
    eq(d2.cumsum(0), a2.cumsum(0))
    eq(d2.sum(1), a2.sum(1))
    eq(d2.T[1:], a2.T[1:])
    eq(d2 + d2.cumsum(1, True), a2 + a2.cumsum(1, True))


def test_from_pointers_wraps_without_a_copy(pks):
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer
    a = residues(pks[1024], (6, 2), 81)
    d = a.to_device()
    w = DeviceCiphertextBuffer.from_pointers(a.public_key, d.data_ptr(), d.exps_ptr(), 12, shape=(6, 2), owner=d,
                                             obfuscated=a.obfuscated)
    assert w.data_ptr() == d.data_ptr() and w.exps_ptr() == d.exps_ptr()
    ref = weakref.ref(d)
    del d
    gc.collect()
    assert ref() is not None                                           # the wrapper keeps its owner alive
    eq(w, a)
    eq(w.cumsum(0), a.cumsum(0))
    w.release()                                                        # frees nothing: it lets go of the owner
    gc.collect()
    assert ref() is None


# ------------------------------------------------------------------------------- re-randomisation and the pool
def _put(pk, rhos):
    """The test's obfuscators into the ring of the key's context, registered like prepare_obfuscators does."""
    from flex.crypto.paillier import _runtime, obfuscator_pool
    ctx = _runtime.context(pk)
    ctx.pool_reserve(len(rhos))
    ctx.pool_put(rhos)
    obfuscator_pool._device[(pk.n, _runtime.device_index(), os.getpid())] = weakref.ref(ctx)
    return ctx


def test_apply_obfuscation(pks, golden):
    from flex.crypto.paillier import _runtime, obfuscator_pool
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey
    pk, key = pks[1024], _key(golden, 1024)
    dec = PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))
    src = PaillierEncryptor(pk).encrypt_to_buffer(np.arange(-5, 7, dtype=np.int64))
    src.obfuscated[[0, 3, 4, 9]] = 0                                  # a partly flagged buffer: the gather path
    rhos = [pow(O.golden_r(key.n, 12, i), key.n, key.nsquare) for i in range(4)]
    try:
        host = src[:]
        _put(pk, rhos)
        host.apply_obfuscation()
        dev = src.to_device()
        _put(pk, rhos)
        assert dev.apply_obfuscation() is dev
        eq(dev, host)                                                  # the same pool entries on both sides: equal bits
        assert dev.obfuscated.all() and not np.array_equal(host.words, src.words)
    finally:
        obfuscator_pool.drop(pk)
    fresh = src.to_device()
    fresh.obfuscated[:] = 0
    before = fresh.to_host().words
    fresh.apply_obfuscation()                                          # fresh r: other bits, the same plaintexts
    after = fresh.to_host().words
    assert fresh.obfuscated.all() and not (after == before).all(axis=1).any()
    assert np.array_equal(dec.decrypt(fresh), np.arange(-5, 7))
    calls = dict(_runtime.context(pk).calls)
    fresh.apply_obfuscation()                                          # every flag set: no GPU call
    assert dict(_runtime.context(pk).calls) == calls and np.array_equal(fresh.to_host().words, after)


# ------------------------------------------------------------------------------- the chain and its traffic
def test_chain_moves_no_ciphertext_between_calls(pks, golden, monkeypatch):
    from flex.crypto.paillier import _runtime, obfuscator_pool
    from flex.crypto.paillier.cipher_array import from_wire
    N = _native()
    pk, key = pks[1024], _key(golden, 1024)
    W = 64
    src = residues(pk, (300,), 91)
    wire = src.to_wire()
    bins, node = _hist_inputs(np.uint8)
    cells = 2 * 3 * 5
    rhos = [pow(O.golden_r(key.n, 13, i), key.n, key.nsquare) for i in range(cells)]
    try:
        _put(pk, rhos)
        hist, wc = from_wire(wire, pk, lazy=True).histogram(bins, 5, node=node, n_nodes=2)
        want = hist.cumsum(axis=2).to_wire(be_secure=True)
        _put(pk, rhos)
        lib = N.load_library()

        def host_entry(*args):
            raise AssertionError("a host-buffer entry point ran inside the device chain")

        for name in ("pai_histogram", "pai_cumsum", "pai_obfuscate", "pai_add", "pai_segment_add"):
            monkeypatch.setattr(lib, name, host_entry)
        enc = from_wire(wire, pk, lazy=True, device=True)
        up0, down0 = N.dev_io_stats()
        hist, gc_ = enc.histogram(bins, 5, node=node, n_nodes=2)
        left = hist.cumsum(axis=2)
        left.apply_obfuscation()
        up1, down1 = N.dev_io_stats()
        got = left.to_wire()
        up2, down2 = N.dev_io_stats()
    finally:
        obfuscator_pool.drop(pk)
    assert got == want and np.array_equal(gc_, wc)
    # in: the bins, the node ids and the cells' exponents; out: counts and exponents; then the cells once
    assert up1 - up0 == bins.nbytes + 300 * 4 + cells * 4 and up1 - up0 < 300 * W * 4
    assert down1 - down0 == cells * 8 + cells * 4
    assert (up2 - up1, down2 - down1) == (0, cells * W * 4 + cells * 4)
    assert _runtime.context(pk).calls["pai_histogram_dev"] >= 1


# ------------------------------------------------------------------------------- lifetime
def test_operands_dropped_while_work_is_queued(pks):
    a, b = residues(pks[2048], (512,), 95), residues(pks[2048], (512,), 96)
    want = a + b
    da, db = a.to_device(), b.to_device()
    c = da + db
    del da, db
    gc.collect()
    eq(c, want)
    e = (c * 3).cumsum()
    del c
    gc.collect()
    eq(e, (want * 3).cumsum())


def test_buffer_outlives_its_context(pks, monkeypatch):
    from flex.crypto.paillier import _runtime
    pk, other = pks[1024], pks[2048]
    a = residues(pk, (5, 4), 97)
    d = a.to_device().cumsum(1)                                        # filled by the key's current context
    old = weakref.ref(_runtime.context(pk))
    monkeypatch.setenv("FLEXPAI_MAX_CONTEXTS", "1")
    _runtime.context(other)                                            # the other key's context takes the only place
    with _runtime._lock:
        _runtime._evict_lru()
    gc.collect()
    assert old() is None and all(c.n != pk.n for c in _runtime.cached_contexts())
    eq(d, a.cumsum(1))                                                 # the download needs no context
    eq(d.cumsum(0) + d, a.cumsum(1).cumsum(0) + a.cumsum(1))           # a context made anew
    assert old() is None


# ------------------------------------------------------------------------------- packed buffers
def test_pack_on_the_device(pks):
    from flex.crypto.paillier import parallel_ops
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk = pks[1024]
    lay = PackedLayout(pk, 32, 20, 0)
    src = PaillierEncryptor(pk).encrypt_to_buffer(np.random.default_rng(4).integers(-500, 500, (3, 37)))
    want = src.pack(lay, 500)
    got = src.to_device().pack(lay, 500)
    assert got.resident and not want.resident and got.shape == want.shape and got.bound == want.bound
    assert np.array_equal(got.to_host().words, want.words) and got.to_wire() == want.to_wire()
    bins = np.random.default_rng(5).integers(0, 4, (111, 2)).astype(np.uint8)
    wp, wc = parallel_ops.histogram_packed(src, bins, 4, lay, 500)
    gp, gc_ = parallel_ops.histogram_packed(src.to_device(), bins, 4, lay, 500)
    assert gp.resident and np.array_equal(gc_, wc) and np.array_equal(gp.to_host().words, wp.words)
    assert (gp.shape, gp.bound, gp.count) == (wp.shape, wp.bound, wp.count)


def test_host_exponents_of_the_packed_paths(pks, golden):
    """The paths that hand HOST exponents to a device call (the uniform exponents of a resident packed buffer, the source
    exponents of pack): the uploaded block has to live through the call. Mixed source exponents decide pack's slot
    shifts, so wrong exponents change the bits."""
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, key = pks[1024], _key(golden, 1024)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))
    rng = np.random.default_rng(8)
    enc0 = enc.encrypt_to_buffer(rng.integers(-500, 500, 3000))
    src = CiphertextBuffer(pk, enc0.words, rng.integers(0, 3, 3000).astype(np.int32), 1, (3000,))
    lay = PackedLayout(pk, 32, 20, 2)
    want = src.pack(lay, 500)
    got = src.to_device().pack(lay, 500)
    assert got.resident and got.bound == want.bound and np.array_equal(got.to_host().words, want.words)
    with pytest.raises(ValueError, match="index 7 has exponent 3"):
        exps = src.exps.copy()
        exps[7] = 3
        CiphertextBuffer(pk, src.words, exps, 1, (3000,)).to_device().pack(lay, 500)
    lay3 = PackedLayout(pk, 32, 14, 3, 2)                              # values at 16^-3: a layout exponent that is not 0
    gh = rng.integers(-4000, 4000, (300, 2)) / 4096.0
    host = enc.encrypt_packed(gh, lay3)
    dev = host.to_device()
    bins, node = _hist_inputs(np.uint16)
    for buf in (host, dev):
        hist, cnt = buf.histogram(bins, 5, node=node, n_nodes=2)
        out = (hist.cumsum(axis=0, reverse=True) * 2 - hist).take([2, 0], axis=1)
        if buf is host:
            want, wc = out, cnt
    assert out.resident and np.array_equal(cnt, wc) and np.array_equal(out.to_host().words, want.words)
    assert (out.shape, out.bound) == (want.shape, want.bound) and np.array_equal(dec.decrypt(out), dec.decrypt(want))
    sums = dec.decrypt(hist.to_host() if hist.resident else hist)
    assert np.allclose(sums[1, 0, 2], gh[(node == 1) & (bins[:, 0] == 2)].sum(axis=0), rtol=0, atol=1e-9)


def test_packed_chain(pks, golden):
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    pk, key = pks[1024], _key(golden, 1024)
    dec = PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))
    lay = PackedLayout(pk, 32, 12, 0, 2)                               # g and h of a sample in two slots
    gh = np.random.default_rng(6).integers(-1000, 1000, (300, 2))
    host = PaillierEncryptor(pk).encrypt_packed(gh, lay)
    dev = host.to_device()
    assert dev.resident and dev.to_device() is dev and np.array_equal(dev.to_host().words, host.words)
    bins, node = _hist_inputs(np.uint8)

    def chain(buf):
        hist, cnt = buf.histogram(bins, 5, node=node, n_nodes=2)
        left = hist.cumsum(axis=2)
        return hist, cnt, left, left + left, left - hist, (left * -3).take([1, 0, 1], axis=1)

    want, got = chain(host), chain(dev)
    assert np.array_equal(got[1], want[1])
    for g, w in zip(got[:1] + got[2:], want[:1] + want[2:]):
        assert g.resident and not w.resident
        assert (g.shape, g.bound, g.count, g.obfuscated) == (w.shape, w.bound, w.count, w.obfuscated)
        assert np.array_equal(g.to_host().words, w.words)
        assert np.array_equal(dec.decrypt(g), dec.decrypt(w))
    mixed = got[2] + want[2]                                           # a host operand is uploaded for the call
    assert mixed.resident and np.array_equal(mixed.to_host().words, want[3].words)
    wire = want[2].to_wire()
    assert got[2].to_wire() == wire
    back = PackedCiphertextBuffer.from_wire(wire, pk, device=True)
    assert back.resident and np.array_equal(back.to_host().words, want[2].words) and back.bound == want[2].bound
    sealed = got[4].apply_obfuscation()
    assert sealed.obfuscated and not np.array_equal(sealed.to_host().words, want[4].words)
    assert np.array_equal(dec.decrypt(sealed), dec.decrypt(want[4]))
    with pytest.raises(OverflowError):                                 # the bound is checked before any GPU call
        got[2] * (1 << 20)
    bad = want[2].words.copy()
    bad[3] = _native().ints_to_words([pk.nsquare + 5], bad.shape[1])[0]
    corrupt = PackedCiphertextBuffer(pk, bad, lay, want[2].count, want[2].shape, False, want[2].bound).to_wire()
    for device in (False, True):
        with pytest.raises(ValueError, match=r"ciphertext >= n\^2"):
            PackedCiphertextBuffer.from_wire(corrupt, pk, device=device)


# ------------------------------------------------------------------------------- the key holder
@pytest.mark.parametrize("nb", [1024, 2048, 4096])
def test_encrypt_to_device_and_decrypt(golden, nb):
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey
    key = _key(golden, nb)
    pk = _pk(key)
    enc, dec = PaillierEncryptor(pk), PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))
    rng = np.random.default_rng(nb)
    n = 5 if nb == 4096 else 33
    f64 = np.concatenate([[0.0, -0.0, 2.0 ** 60 + 1, -123.456, 1.0 / 3.0], rng.standard_normal(n)])[:max(n, 5)]
    for x in (rng.standard_normal(n).astype(np.float32).reshape(-1, 1), f64,
              np.array([0, 1, -1, 2 ** 62, -(2 ** 62), 123456789], dtype=np.int64)[:max(n, 5)]):
        buf = enc.encrypt_to_buffer(x, device=True)
        assert isinstance(buf, DeviceCiphertextBuffer) and buf.shape == x.shape and buf.obfuscated.all()
        got = dec.decrypt(buf)
        assert got.shape == x.shape
        if x.dtype == np.float64:
            # a float64 keeps at least 50 of its 53 bits through the base-16 encoder (4 e <= 53 - fe), the bound of
            # tests/test_gpu_obfuscate.py; the bits contract itself is the comparison with the host path below
            assert np.allclose(got, x, rtol=2.0 ** -49, atol=0.0)
        else:
            assert np.array_equal(got, x.astype(got.dtype))
        host = dec.decrypt(buf.to_host())
        assert got.dtype == host.dtype and np.array_equal(got, host)
    # statuses: a sum that leaves the float range, through both decrypt paths
    tiny = enc.encrypt_to_buffer(np.array([1e-300, -1e-300, 5e-324]), device=True)
    assert np.array_equal(dec.decrypt(tiny), dec.decrypt(tiny.to_host()))
    mixed = residues(pk, (5,), nb)
    for buf in (mixed, mixed.to_device()):
        try:
            out = dec.decrypt(buf)
        except OverflowError as e:
            out = str(e)
        if buf is mixed:
            want = out
    assert repr(out) == repr(want)
    with pytest.raises(ValueError, match="different key"):
        dec.decrypt(residues(_pk(_key(golden, 2048 if nb != 2048 else 1024)), (2,), 1).to_device())
