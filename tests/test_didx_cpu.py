"""DeviceArray and the calls that accept it, without a GPU: the package's usual RuntimeError, the dtype and shape refusals
before any native call, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from flex.crypto.paillier import _native, _runtime
from flex.crypto.paillier.device_buffer import (DeviceArray, DeviceCiphertextBuffer, DeviceWords, device_array)
from flex.crypto.paillier.keypair import PaillierPublicKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = "CiphertextBuffer operators need a GPU"
N_S = 12


@pytest.fixture(scope="module")
def pk(golden):
    return PaillierPublicKey(int(golden["keys"]["1024"]["n"], 16))


def named(dtype, shape, at=1 << 20):
    """A DeviceArray over an address nothing reads: the constructor makes no native call."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return DeviceArray(_native.DeviceMem.wrap(at, n, 0), dtype, shape)


@pytest.fixture()
def buf(pk):
    W = (2 * pk.n.bit_length() + 31) // 32
    words = DeviceWords(_native.DeviceMem.wrap(1 << 24, N_S * W * 4, 0), N_S, W)
    return DeviceCiphertextBuffer(pk, words, _native.DeviceMem.wrap(1 << 25, N_S * 4, 0))


@pytest.fixture()
def no_gpu(monkeypatch):
    monkeypatch.setattr(_runtime, "_gpus", (os.getpid(), 0))          # a process that sees no GPU
    assert not _runtime.gpu_available()


def test_device_array_describes_its_block():
    a = named(np.int64, (3, 4))
    assert (a.shape, a.size, a.ndim, a.nbytes, a.dtype, a.ptr, a.device) == ((3, 4), 12, 2, 96, np.int64, 1 << 20, 0)
    assert named(np.uint8, 5).shape == (5,) and named(np.int32, ()).size == 1
    with pytest.raises(ValueError, match="does not hold"):
        DeviceArray(_native.DeviceMem.wrap(1 << 20, 95, 0), np.int64, (3, 4))
    with pytest.raises(ValueError, match="bad shape"):
        DeviceArray(_native.DeviceMem.wrap(1 << 20, 95, 0), np.int64, (-1,))


def test_device_operands_need_a_gpu(buf, no_gpu):
    with pytest.raises(RuntimeError, match=NO_GPU):
        device_array(np.arange(4))
    with pytest.raises(RuntimeError, match=NO_GPU):
        DeviceArray.from_pointer(4096, np.int64, (4,))
    idx, off = named(np.int64, (5,)), named(np.int64, (3,))
    for call in (lambda: buf.take(idx), lambda: buf[idx], lambda: buf.segment_sum(idx, off),
                 lambda: buf.segment_sum(np.arange(5), off), lambda: buf.segment_sum(np.arange(5), np.array([0, 2, 5])),
                 lambda: buf.histogram(named(np.uint8, (N_S, 3)), 4),
                 lambda: buf.histogram(np.zeros((N_S, 3), dtype=np.uint8), 4, node=named(np.int32, (N_S,)), n_nodes=2)):
        with pytest.raises(RuntimeError, match=NO_GPU):
            call()


def test_refusals_come_before_any_native_call(buf, pk, monkeypatch):
    calls = []

    def boom(*a, **k):
        calls.append(1)
        raise AssertionError("refused arguments must not reach the runtime")
    monkeypatch.setattr(_runtime, "context", boom)
    monkeypatch.setattr(_runtime, "gpu_available", boom)
    monkeypatch.setattr(_native, "device_upload", boom)
    monkeypatch.setattr(_native.Context, "dev_call", boom)
    bins, node = named(np.uint8, (N_S, 3)), named(np.int32, (N_S,))
    host_bins = np.zeros((N_S, 6), dtype=np.uint8)
    refused = [
        (TypeError, "int64", lambda: buf.take(named(np.float64, (5,)))),
        (TypeError, "int64", lambda: buf[named(np.int32, (5,))]),
        (ValueError, "axis", lambda: buf.take(named(np.int64, (5,)), axis=0)),
        (TypeError, "int64", lambda: buf.segment_sum(named(np.float32, (5,)), np.array([0, 5]))),
        (TypeError, "integers", lambda: buf.segment_sum(named(np.int64, (5,)), np.array([0.0, 5.0]))),
        (ValueError, "one-dimensional", lambda: buf.segment_sum(named(np.int64, (5, 1)), np.array([0, 5]))),
        (ValueError, "one-dimensional", lambda: buf.segment_sum(np.arange(5), named(np.int64, (2, 1)))),
        (ValueError, "must start at 0", lambda: buf.segment_sum(named(np.int64, (5,)), named(np.int64, (0,)))),
        (TypeError, "uint8 or uint16", lambda: buf.histogram(named(np.int32, (N_S, 3)), 4)),
        (ValueError, "must have shape", lambda: buf.histogram(named(np.uint8, (N_S,)), 4)),
        (ValueError, "must have shape", lambda: buf.histogram(named(np.uint8, (N_S + 1, 3)), 4)),
        (ValueError, "n_bins must be in", lambda: buf.histogram(bins, 257)),
        (ValueError, "n_nodes must be 1", lambda: buf.histogram(bins, 4, n_nodes=2)),
        (TypeError, "int32", lambda: buf.histogram(bins, 4, node=named(np.int64, (N_S,)), n_nodes=2)),
        (ValueError, "node must have shape", lambda: buf.histogram(bins, 4, node=named(np.int32, (N_S, 1)), n_nodes=2)),
        (ValueError, "node must have shape", lambda: buf.histogram(bins, 4, node=np.zeros((N_S, 1), dtype=np.int32),
                                                                    n_nodes=2)),
        (ValueError, "contiguous", lambda: buf.histogram(host_bins[:, ::2], 4, node=node, n_nodes=2)),
        (TypeError, "uint8 or uint16", lambda: buf.histogram(host_bins.astype(np.int16), 4, node=node, n_nodes=2)),
    ]
    for exc, text, call in refused:
        with pytest.raises(exc, match=text):
            call()
    assert not calls
    # the packed buffer: DeviceArray operands on a buffer that is not resident, and shape refusals on one that is
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    lay = PackedLayout(pk, 32, 20, 0, 2)
    W = buf.words.shape[1]
    host = PackedCiphertextBuffer(pk, np.zeros((N_S, W), dtype=np.uint32), lay, 2 * N_S, (N_S, 2))
    with pytest.raises(TypeError, match="resident buffer"):
        host.histogram(bins, 4)
    resident = PackedCiphertextBuffer(pk, buf.words, lay, 2 * N_S, (N_S, 2), False, 1)
    assert resident.resident
    with pytest.raises(ValueError, match="node must have shape"):
        resident.histogram(bins, 4, node=named(np.int32, (N_S, 1)), n_nodes=2)
    big = PackedCiphertextBuffer(pk, buf.words, lay, 2 * N_S, (N_S, 2), False, lay.slot_max // 2)
    with pytest.raises(OverflowError, match="cannot be counted on the host"):
        big.histogram(bins, 4)
    assert not calls


def test_the_header_declares_and_the_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "flexpai.h")).read()
    for name in _native.DEVICE_INDEX:
        assert name in _native.EXPORTED and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert _native.DEVICE_INDEX == ("pai_take_idx_dev", "pai_segment_add_idx_dev")
    assert set(_native.RESIDENT) == {"pai_dev_alloc", "pai_dev_free", "pai_dev_upload", "pai_dev_download", "pai_dev_copy",
                                     "pai_dev_io_stats", "pai_dev_release_staging", "pai_take_dev", "pai_check_below_dev"}
