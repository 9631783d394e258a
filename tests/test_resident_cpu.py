"""Indexing, take, concatenate and transpose of CiphertextBuffer against numpy on the materialised array (no GPU), and
the device entry points' RuntimeError without one."""
import os

import numpy as np
import pytest

from flex.crypto.paillier import _native, _runtime
from flex.crypto.paillier.cipher_array import from_wire
from flex.crypto.paillier.cipher_buffer import CiphertextBuffer, concatenate
from flex.crypto.paillier.encryptor import PaillierEncryptor
from flex.crypto.paillier.keypair import PaillierPublicKey

NO_GPU = "CiphertextBuffer operators need a GPU"


@pytest.fixture(scope="module")
def pk(golden):
    return PaillierPublicKey(int(golden["keys"]["1024"]["n"], 16))


def residues(pk, shape, seed):
    """Random residues mod n^2 with exponents 0..20 and mixed obfuscation flags."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    W = (2 * pk.n.bit_length() + 31) // 32
    words = _native.ints_to_words([int.from_bytes(rng.bytes(4 * W), "little") % pk.nsquare for _ in range(N)], W)
    return CiphertextBuffer(pk, words, rng.integers(0, 21, N).astype(np.int32), rng.integers(0, 2, N).astype(np.uint8), shape)


@pytest.fixture(scope="module")
def cube(pk):
    return residues(pk, (4, 7, 3), 11)


@pytest.fixture(scope="module")
def flat(pk):
    return residues(pk, (37,), 12)


def same(buf, want):
    """buf (a CiphertextBuffer) against an object array or one PaillierEncryptedNumber: shape, bits, exponents, flags."""
    got = np.asarray(buf.to_array())
    want = np.asarray(want, dtype=object)
    assert got.shape == want.shape == buf.shape
    for g, w in zip(got.reshape(-1), want.reshape(-1)):
        assert g.ciphertext(False) == w.ciphertext(False) and g.exponent == w.exponent
        assert g._is_obfuscated() == w._is_obfuscated()
    assert buf.words.shape[0] == buf.exps.size == buf.obfuscated.size == got.size


def keys_for(buf):
    mask = np.random.default_rng(5).integers(0, 2, buf.shape[0]).astype(bool)
    return [2, -1, slice(1, 3), slice(None, None, -2), (Ellipsis, 0), [[0, 3, 3]], ([0, 3, 3],), mask, slice(3, 3),
            np.zeros(buf.shape[0], dtype=bool), (None, slice(0, 2))]


@pytest.mark.parametrize("which", ["cube", "flat"])
def test_getitem_follows_numpy(which, cube, flat):
    buf = cube if which == "cube" else flat
    arr = np.asarray(buf.to_array())
    for key in keys_for(buf):
        same(buf[key], arr[key])
    if which == "cube":
        same(buf[1, 2:5, [0, 2]], arr[1, 2:5, [0, 2]])
        same(buf[3, 6, 2], arr[3, 6, 2])
        assert buf[3, 6, 2].shape == () and buf[3, 6, 2].size == 1
    with pytest.raises(IndexError):
        buf[buf.shape[0]]


def test_take_concatenate_transpose(cube, flat):
    arr = np.asarray(cube.to_array())
    same(cube.take([6, 0, 0, -2], axis=1), np.take(arr, [6, 0, 0, -2], axis=1))
    same(cube.take([[83, 0], [5, 5]]), np.take(arr, [[83, 0], [5, 5]]))
    same(flat.take([], axis=0), np.take(np.asarray(flat.to_array()), [], axis=0))
    same(cube.T, arr.T)
    same(cube.transpose(1, 0, 2), arr.transpose(1, 0, 2))
    same(cube.transpose((2, 0, 1)), arr.transpose(2, 0, 1))
    other = residues(cube.public_key, (2, 7, 3), 13)
    same(concatenate([cube, other, cube]), np.concatenate([arr, np.asarray(other.to_array()), arr]))
    wide = residues(cube.public_key, (4, 7, 5), 14)
    same(concatenate([cube, wide], axis=2), np.concatenate([arr, np.asarray(wide.to_array())], axis=2))
    same(concatenate([flat]), np.asarray(flat.to_array()))
    with pytest.raises(ValueError):
        concatenate([cube, wide], axis=0)
    with pytest.raises(ValueError):
        concatenate([cube, residues(PaillierPublicKey(cube.public_key.n + 2), (1, 7, 3), 1)])


def test_selection_copies(flat):
    part = flat[3:9]
    part.obfuscated[:] = 1
    part.exps[:] = 99
    assert flat.exps.max() <= 20 and np.array_equal(flat.obfuscated[3:9], residues(flat.public_key, (37,), 12).obfuscated[3:9])


def test_device_entry_points_need_a_gpu(pk, flat, monkeypatch):
    monkeypatch.setattr(_runtime, "_gpus", (os.getpid(), 0))          # a process that sees no GPU
    assert not _runtime.gpu_available()
    with pytest.raises(RuntimeError, match=NO_GPU):
        flat.to_device()
    with pytest.raises(RuntimeError, match=NO_GPU):
        from_wire(flat.to_wire(), pk, lazy=True, device=True)
    with pytest.raises(RuntimeError, match=NO_GPU):
        PaillierEncryptor(pk).encrypt_to_buffer(np.arange(4.0), device=True)
    from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer
    with pytest.raises(RuntimeError, match=NO_GPU):
        DeviceCiphertextBuffer.from_pointers(pk, 4096, 8192, 1)
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    lay = PackedLayout(pk, 32, 20, 0, 2)
    packed = PackedCiphertextBuffer(pk, flat.words[:3], lay, 6, (3, 2))
    with pytest.raises(RuntimeError, match=NO_GPU):
        packed.to_device()
    with pytest.raises(RuntimeError, match=NO_GPU):
        PackedCiphertextBuffer.from_wire(packed.to_wire(), pk, device=True)
    assert not packed.resident and packed.take([2, 0], axis=0).shape == (2, 2)


def test_from_wire_device_needs_lazy(pk, flat):
    with pytest.raises(ValueError, match="lazy=True"):
        from_wire(flat.to_wire(), pk, device=True)
