"""DeviceArray operands of DeviceCiphertextBuffer and the resident PackedCiphertextBuffer: take / buf[idx] / segment_sum
over an index that is device memory, and histogram over resident bins and node ids, against the host-operand calls on
the same inputs (same words, same decryption); the flag rule; the errors; and the traffic contract."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
N_S, F, B, NODES = 300, 3, 5, 2


def _native():
    from flex.crypto.paillier import _native as N
    return N


@pytest.fixture(scope="module")
def party(golden):
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.encryptor import PaillierEncryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    pk = PaillierPublicKey(key.n)
    return pk, PaillierEncryptor(pk), PaillierDecryptor(pk, PaillierPrivateKey(pk, key.p, key.q))


@pytest.fixture(scope="module")
def data(party):
    """300 encrypted float64 values of mixed sign and magnitude (so of mixed exponents) on the device, with bins, node
    ids and index lists for them."""
    _, enc, _ = party
    rng = np.random.default_rng(21)
    x = rng.standard_normal(N_S) * 10.0 ** rng.integers(-3, 4, N_S)
    dev = enc.encrypt_to_buffer(x).to_device()
    assert np.unique(dev.exps).size > 2
    bins = rng.integers(0, B, (N_S, F)).astype(np.uint8)
    node = rng.integers(-1, NODES + 1, N_S).astype(np.int32)            # some samples in no node
    idx = rng.integers(0, N_S, (7, 45)).astype(np.int64)
    lens = np.array([0, 1, 17, 40, 0, 257], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return x, dev, bins, node, idx, off


def same(a, b):
    assert a.shape == b.shape
    ha, hb = a.to_host(), b.to_host()
    assert np.array_equal(ha.words, hb.words) and np.array_equal(ha.exps, hb.exps)


def test_take_getitem_and_segment_sum(party, data):
    from flex.crypto.paillier.device_buffer import device_array
    _, _, dec = party
    x, dev, _, _, idx, off = data
    d_idx = device_array(idx)
    assert d_idx.shape == idx.shape and np.array_equal(d_idx.to_host(), idx)
    want = dev.take(idx)
    for got in (dev.take(d_idx), dev[d_idx]):
        same(got, want)
        assert np.array_equal(dec.decrypt(got), dec.decrypt(want))
        assert np.allclose(dec.decrypt(got), x[idx], rtol=1e-12, atol=0)      # (the float encoding keeps 53 bits or so)
    assert dev.take(device_array(np.zeros(0, dtype=np.int64))).shape == (0,)
    flat = idx.reshape(-1)
    d_flat, d_off = device_array(flat), device_array(off)
    want = dev.segment_sum(flat, off)                                   # pai_segment_add_dev
    assert want.shape == (off.size - 1,) and want.exps[0] == 0 and want.exps[4] == 0      # the empty segments
    for a, b in ((d_flat, d_off), (flat, d_off), (d_flat, off)):
        same(dev.segment_sum(a, b), want)
    sums = dec.decrypt(want)
    for s in range(off.size - 1):
        assert sums[s] == pytest.approx(x[flat[off[s]:off[s + 1]]].sum(), rel=1e-9, abs=1e-12)
    same(dev.sum(), dev.segment_sum(device_array(np.arange(N_S, dtype=np.int64)), np.array([0, N_S])))


def test_flags_of_a_device_take(data):
    """The flags are a host array and the index is not on the host: obfuscated only when every source flag is set."""
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer, device_array
    _, dev, _, _, idx, _ = data
    d_idx = device_array(idx)
    mixed = DeviceCiphertextBuffer(dev.public_key, dev.words, dev._ex, (np.arange(N_S) % 2).astype(np.uint8))
    sealed = DeviceCiphertextBuffer(dev.public_key, dev.words, dev._ex, 1)
    assert not mixed.take(d_idx).obfuscated.any() and not mixed[d_idx].obfuscated.any()
    assert sealed.take(d_idx).obfuscated.all() and sealed.take(d_idx).obfuscated.shape == (idx.size,)
    assert dev.obfuscated.all() and dev.take(d_idx).obfuscated.all()   # a freshly encrypted buffer: every flag is set
    bare = DeviceCiphertextBuffer(dev.public_key, dev.words, dev._ex, 0)
    assert not bare.take(d_idx).obfuscated.any()
    assert not sealed.segment_sum(device_array(idx.reshape(-1)), np.array([0, idx.size])).obfuscated.any()


def test_bad_lists_raise(data):
    from flex.crypto.paillier.device_buffer import device_array
    _, dev, _, _, idx, off = data
    bad = idx.copy()
    bad[3, 11] = N_S
    bad[5, 0] = -1
    pos = 3 * idx.shape[1] + 11
    with pytest.raises(IndexError, match=f"position {pos} is out of bounds for {N_S}"):
        dev.take(device_array(bad))
    with pytest.raises(IndexError, match=f"position {pos} "):
        dev[device_array(bad)]
    flat = idx.reshape(-1)
    with pytest.raises(IndexError, match=f"segment_sum: index out of range for {N_S}"):
        dev.segment_sum(device_array(bad.reshape(-1)), off)
    for wrong, text in ((off + 1, "must start at 0"), (off[::-1].copy(), "must start at 0"),
                        (np.concatenate([off[:3], [0], off[4:]]), "must not decrease"),
                        (off[:-1], f"{flat.size} indices, seg_off ends at {int(off[-2])}")):
        errors = []
        for o in (wrong, device_array(wrong)):                          # the host check and the device check say the same
            with pytest.raises(ValueError, match=text) as e:
                dev.segment_sum(flat, o)
            errors.append(str(e.value))
        assert errors[0] == errors[1]
    with pytest.raises(TypeError, match="int64"):
        dev.take(device_array(idx.astype(np.int32)))
    with pytest.raises(ValueError, match="axis"):
        dev.take(device_array(idx), axis=0)
    same(dev.take(device_array(flat)), dev.take(flat))                  # and the buffer still serves


def test_histogram_on_resident_operands(party, data):
    from flex.crypto.paillier.device_buffer import device_array
    from flex.crypto.paillier.packed_buffer import PackedLayout
    pk, enc, dec = party
    _, dev, bins, node, _, _ = data
    d_bins, d_node = device_array(bins), device_array(node)
    want, wc = dev.histogram(bins, B, node=node, n_nodes=NODES)
    for b, nd in ((d_bins, d_node), (d_bins, node), (bins, d_node)):
        got, cnt = dev.histogram(b, B, node=nd, n_nodes=NODES)
        same(got, want)
        assert np.array_equal(cnt, wc)
    same(dev.histogram(d_bins, B)[0], dev.histogram(bins, B)[0])
    wide = bins.astype(np.uint16)
    same(dev.histogram(device_array(wide), B, node=d_node, n_nodes=NODES)[0], want)
    # the resident packed buffer: one ciphertext per sample, g and h in two slots
    lay = PackedLayout(pk, 32, 14, 3, 2)
    gh = np.random.default_rng(2).integers(-4000, 4000, (N_S, 2)) / 4096.0
    packed = enc.encrypt_packed(gh, lay).to_device()
    ph, pc = packed.histogram(bins, B, node=node, n_nodes=NODES)
    gh_, gc = packed.histogram(d_bins, B, node=d_node, n_nodes=NODES)
    assert gh_.resident and gh_.bound == ph.bound and gh_.shape == ph.shape and np.array_equal(gc, pc)
    assert np.array_equal(gh_.to_host().words, ph.to_host().words)
    assert np.array_equal(dec.decrypt(gh_), dec.decrypt(ph))
    with pytest.raises(TypeError, match="resident buffer"):
        packed.to_host().histogram(d_bins, B, node=d_node, n_nodes=NODES)


def test_resident_operands_add_no_upload(data):
    """After bins, node and the index lists have been uploaded once, a round of histogram + take + segment_sum moves
    up only what the calls themselves still upload: the exponents of a result built from host exponents (histogram and
    segment_sum set the empty cells' exponents on the host), 4 bytes per result element. The bins (N F bytes), the node
    ids (4 N) and the lists (8 bytes per entry) alone would be more than that."""
    from flex.crypto.paillier.device_buffer import device_array
    N = _native()
    _, dev, bins, node, idx, off = data
    flat = idx.reshape(-1)
    d_bins, d_node, d_idx, d_flat, d_off = (device_array(a) for a in (bins, node, idx, flat, off))

    def round_():
        hist, _ = dev.histogram(d_bins, B, node=d_node, n_nodes=NODES)
        return hist, dev.take(d_idx), dev.segment_sum(d_flat, d_off)
    round_()                                                            # warm: contexts, scratch
    up0, down0 = N.dev_io_stats()
    hist, took, sums = round_()
    up1, down1 = N.dev_io_stats()
    cells, nseg = NODES * F * B, off.size - 1
    allowed = 4 * cells + 4 * nseg
    assert up1 - up0 <= allowed < min(bins.nbytes, node.nbytes, idx.nbytes, flat.nbytes)
    # down: the counts and exponents of the histogram, the check words of take and segment_sum, the sums' exponents
    assert down1 - down0 == 8 * cells + 4 * cells + 16 + 16 + 4 * nseg
    same(took, dev.take(idx))
    same(sums, dev.segment_sum(flat, off))
    same(hist, dev.histogram(bins, B, node=node, n_nodes=NODES)[0])


def test_an_index_made_by_torch_on_the_device(data):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch device")
    from flex.crypto.paillier.device_buffer import DeviceArray
    _, dev, _, node, _, _ = data
    t_node = torch.from_numpy(node).to(torch.device("cuda", dev.device))
    picked = torch.nonzero(t_node == 1).reshape(-1)                     # int64, made on the device
    torch.cuda.synchronize()
    d_idx = DeviceArray.from_pointer(picked.data_ptr(), np.int64, tuple(picked.shape), owner=picked, device=dev.device)
    host_idx = picked.cpu().numpy()
    assert host_idx.size and np.array_equal(host_idx, np.flatnonzero(node == 1))
    same(dev.take(d_idx), dev.take(host_idx))
    same(dev.segment_sum(d_idx, np.array([0, host_idx.size])), dev.segment_sum(host_idx, np.array([0, host_idx.size])))
    assert d_idx.mem.owner is picked
