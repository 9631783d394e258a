"""DeviceCiphertextBuffer: a CiphertextBuffer whose words and exponents stay on the GPU between calls.

CiphertextBuffer (cipher_buffer.py) keeps its words in numpy, so every operator uploads its operands and downloads its
result: each link of a chain crosses PCIe twice. A DeviceCiphertextBuffer holds them in device memory of the library
(pai_dev_alloc: owned by the device, not by a context, so a buffer outlives the context that filled it) and runs the same
kernels through the *_dev entry points of include/flexpai.h:

    enc_gh = from_wire(received, lazy=True, device=True)     # parse, ONE upload, range check on the device
    hist, counts = enc_gh.histogram(bins, n_bins, node=node_of_sample, n_nodes=n_open)
    left = hist.cumsum(axis=2)                               # no ciphertext word crosses PCIe in between
    send(left.to_wire(be_secure=True))                       # ONE download

What crosses per call: plain operands in (bins, node ids, scalars, matrices, index lists), counts, statuses and exponents
out. Every result equals the host class's bit for bit (same kernels); the obfuscation flags stay a host array. The package
never imports torch: a caller that already holds device memory wraps it with DeviceCiphertextBuffer.from_pointers(...,
owner=tensor) and reads .data_ptr() / .exps_ptr() for the way back.

Plain operands can stay on the device too: a DeviceArray (device_array(np_array), or DeviceArray.from_pointer(...,
owner=tensor) for memory somebody else made) is accepted as the int64 index of take / buf[idx] / segment_sum
(pai_take_idx_dev, pai_segment_add_idx_dev: checked on the device, nothing goes up) and as the dense bins and the node
ids of histogram, so that a training run uploads its bins once.

This module also holds the word-level device calls (DeviceWords in, DeviceWords out) that cipher_buffer's *_words helpers
hand a device holder to, which is how PackedCiphertextBuffer.to_device() gets its residency from the same place.

Dropping a buffer while kernels that read it are still queued is safe: a block's finaliser waits for the device
(pai_dev_free). release() frees now; views made by reshape() share the block and end with it.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

from . import _native
from .cipher_buffer import (EMPTY_EXP, BufferOps, CiphertextBuffer, _plain, axis_split, histogram_args,
                            histogram_sparse_args, need_gpu, segment_dot_args, sparse_csr)
from .encrypted_number import PaillierEncryptedNumber


class DeviceWords(object):
    """[N, W] ciphertext words in a device block: the device holder the word-level helpers accept next to numpy words."""
    __slots__ = ("mem", "shape")

    def __init__(self, mem: "_native.DeviceMem", N: int, W: int):
        if mem.nbytes < int(N) * int(W) * 4:
            raise ValueError(f"device block of {mem.nbytes} bytes does not hold ({N}, {W}) words")
        self.mem, self.shape = mem, (int(N), int(W))

    @classmethod
    def empty(cls, N: int, W: int, device: int) -> "DeviceWords":
        return cls(_native.DeviceMem(int(N) * int(W) * 4, device), N, W)

    @classmethod
    def from_host(cls, words: np.ndarray, device: int) -> "DeviceWords":
        words = np.ascontiguousarray(words, dtype=np.uint32)
        return cls(_native.device_upload(words, device), words.shape[0], words.shape[1])

    @property
    def ptr(self) -> int:
        return self.mem.ptr

    @property
    def device(self) -> int:
        return self.mem.device

    def to_host(self) -> np.ndarray:
        N, W = self.shape
        return self.mem.download(np.uint32, N * W).reshape(N, W)


class DeviceArray(object):
    """A typed plain operand on the device: a DeviceMem, a dtype and a shape (C-contiguous). device_array(a) uploads a
    numpy array once; DeviceArray.from_pointer wraps memory somebody else owns."""
    __slots__ = ("mem", "dtype", "shape")

    def __init__(self, mem: "_native.DeviceMem", dtype, shape):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        if any(v < 0 for v in self.shape):
            raise ValueError(f"DeviceArray: bad shape {self.shape}")
        if mem.nbytes < self.nbytes:
            raise ValueError(f"device block of {mem.nbytes} bytes does not hold {self.shape} of {self.dtype}")
        self.mem = mem

    @classmethod
    def from_pointer(cls, ptr: int, dtype, shape, owner=None, device: Optional[int] = None) -> "DeviceArray":
        """Wrap device memory somebody else owns (a torch tensor's data_ptr(), C-contiguous), without a copy. `owner` is
        kept alive as long as the array; nothing is freed. The memory must be complete before the first call that reads
        it: the library queues its work on the null stream and knows nothing of the stream that wrote it."""
        from . import _runtime
        need_gpu()
        dev = _runtime.device_index() if device is None else int(device)
        dt = np.dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        return cls(_native.DeviceMem.wrap(ptr, n * dt.itemsize, dev, owner), dt, shape)

    @property
    def ptr(self) -> int:
        return self.mem.ptr

    @property
    def device(self) -> int:
        return self.mem.device

    @property
    def size(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def nbytes(self) -> int:
        return self.size * self.dtype.itemsize

    def to_host(self) -> np.ndarray:
        """One download (waits for the device's queued work)."""
        return self.mem.download(self.dtype, self.size).reshape(self.shape)

    def __repr__(self) -> str:
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, device={self.device})"


def device_array(a, device: Optional[int] = None) -> DeviceArray:
    """The numpy array `a` (made C-contiguous) as a DeviceArray: ONE upload, on `device` or the process's device."""
    from . import _runtime
    need_gpu()
    a = np.ascontiguousarray(a)
    dev = _runtime.device_index() if device is None else int(device)
    return DeviceArray(_native.device_upload(a, dev), a.dtype, a.shape)


def _index_operand(who: str, x, name: str):
    """A take / segment_sum list as it came: a DeviceArray (int64, any shape for take) or a host integer array."""
    if isinstance(x, DeviceArray):
        if x.dtype != np.int64:
            raise TypeError(f"{who}: a device {name} must be int64, not {x.dtype}")
        return x
    a = np.asarray(x)
    if a.dtype.kind not in "iu" and a.size:
        raise TypeError(f"{who}: {name} must hold integers")
    return a.astype(np.int64)


def ct_words(public_key) -> int:
    return (2 * public_key.n.bit_length() + 31) // 32


def context_on(public_key, device: int, private_key=None):
    """This process's context of the key, which must sit on the buffer's device."""
    from . import _runtime
    need_gpu()
    ctx = _runtime.context(public_key, private_key)
    if ctx.device != device:
        raise ValueError(f"the buffer lives on device {device}, the key's context on device {ctx.device}")
    return ctx


def _exp_mem(exps, N: int, device: int) -> "_native.DeviceMem":
    """Exponents as a device block: a DeviceMem as it is, host exponents uploaded for the call (4 bytes each). The caller
    binds the result to a name that lives until its entry point has returned: an unnamed block is freed as soon as its
    .ptr has been read, before the call that takes the pointer."""
    if isinstance(exps, _native.DeviceMem):
        return exps
    return _native.device_upload(np.ascontiguousarray(exps, dtype=np.int32).reshape(N), device)


def _i32(device: int, n: int) -> "_native.DeviceMem":
    return _native.DeviceMem(int(n) * 4, device)


# ---------------------------------------------------------------------- word-level device calls
def add_dev(pk, words: Sequence[DeviceWords], exps: Sequence):
    """pai_add_dev over k operands: (words, exponents). The entry point takes its operands as consecutive arrays, so
    they are gathered by device-to-device copies first."""
    k, (N, W), dev = len(words), words[0].shape, words[0].device
    ctx = context_on(pk, dev)
    ct_all, ex_all = _native.DeviceMem(k * N * W * 4, dev), _i32(dev, k * N)
    for j, (w, e) in enumerate(zip(words, exps)):
        ct_all.copy_from(w.mem, N * W * 4, offset=j * N * W * 4)
        ex_all.copy_from(_exp_mem(e, N, dev), N * 4, offset=j * N * 4)
    out, oe = DeviceWords.empty(N, W, dev), _i32(dev, N)
    ctx.dev_call("pai_add_dev", ct_all.ptr, ex_all.ptr, k, N, out.ptr, oe.ptr)
    return out, oe


def _scalar_call(name: str, pk, words: DeviceWords, exps, x: np.ndarray):
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    x = np.ascontiguousarray(x)
    if x.size not in (1, N):
        raise ValueError("plain operand must have 1 or N elements")
    dx = _native.device_upload(x, dev)
    out, oe, st = DeviceWords.empty(N, W, dev), _i32(dev, N), _i32(dev, N)
    ctx.dev_call(name, words.ptr, ex.ptr, N, _native.scalar_dtype(x), dx.ptr,
                 1 if x.size == N and N > 1 else 0, out.ptr, oe.ptr, st.ptr)
    return out, oe, st.download(np.int32, N)


def mul_dev(pk, words: DeviceWords, exps, x: np.ndarray):
    """pai_mul_dev: (words, exponents, statuses on the host)."""
    return _scalar_call("pai_mul_dev", pk, words, exps, x)


def add_plain_dev(pk, words: DeviceWords, exps, x: np.ndarray):
    """pai_add_plain_dev: (words, exponents, statuses on the host)."""
    return _scalar_call("pai_add_plain_dev", pk, words, exps, x)


def matmul_dev(pk, words: DeviceWords, exps, m: int, K: int, x: np.ndarray, d: int):
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    x = np.ascontiguousarray(x)
    if N != m * K or x.size != K * d:
        raise ValueError("matmul: shape mismatch")
    dx = _native.device_upload(x, dev)
    out, oe = DeviceWords.empty(m * d, W, dev), _i32(dev, m * d)
    ctx.dev_call("pai_matmul_dev", words.ptr, ex.ptr, m, K, _native.scalar_dtype(x), dx.ptr, d,
                 out.ptr, oe.ptr)
    return out, oe


def segment_add_dev(pk, words: DeviceWords, exps, idx: np.ndarray, off: np.ndarray):
    """pai_segment_add_dev (host index lists): (words [nseg, W], exponents). Empty segments: EMPTY_EXP."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    nseg = off.size - 1
    out, oe = DeviceWords.empty(nseg, W, dev), _i32(dev, nseg)
    if nseg > 0:
        ctx.dev_call("pai_segment_add_dev", words.ptr, ex.ptr, N, idx.ctypes.data, off.ctypes.data,
                     nseg, out.ptr, oe.ptr)
    return out, oe


def take_idx_dev(pk, words: DeviceWords, exps, idx: DeviceArray, allow_empty: bool = False):
    """pai_take_idx_dev over an int64 DeviceArray: (words [M, W], exponents [M], the smallest bad position or -1). The
    index does not go up; the two check words (16 bytes) come down."""
    (N, W), dev = words.shape, words.device
    if idx.device != dev:
        raise ValueError(f"the buffer lives on device {dev}, the index on device {idx.device}")
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    M = idx.size
    out, oe, bad = DeviceWords.empty(M, W, dev), _i32(dev, M), _native.DeviceMem(16, dev)
    ctx.take_idx_dev(words.ptr, ex.ptr, N, idx.ptr, M, allow_empty, out.ptr, oe.ptr, bad.ptr)
    return out, oe, int(bad.download(np.int64, 2)[0])


def segment_add_idx_dev(pk, words: DeviceWords, exps, idx: DeviceArray, off: DeviceArray):
    """pai_segment_add_idx_dev over int64 DeviceArrays: (words [nseg, W], exponents, (bad index position, bad offset
    position), each -1 when the lists are good). Empty segments: EMPTY_EXP."""
    (N, W), dev = words.shape, words.device
    if idx.device != dev or off.device != dev:
        raise ValueError(f"the buffer lives on device {dev}, the lists on devices {idx.device} and {off.device}")
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    nseg = off.size - 1
    out, oe, bad = DeviceWords.empty(nseg, W, dev), _i32(dev, nseg), _native.DeviceMem(16, dev)
    ctx.segment_add_idx_dev(words.ptr, ex.ptr, N, idx.ptr, idx.size, off.ptr, nseg, out.ptr, oe.ptr, bad.ptr)
    b = bad.download(np.int64, 2)
    return out, oe, (int(b[0]), int(b[1]))


def segment_dot_dev(pk, words: DeviceWords, exps, idx: np.ndarray, off: np.ndarray, x: np.ndarray):
    """pai_segment_dot_dev: (words [nseg, W], exponents, statuses [nnz] on the host)."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    x = np.ascontiguousarray(x)
    nseg = off.size - 1
    out, oe, st = DeviceWords.empty(nseg, W, dev), _i32(dev, nseg), _i32(dev, idx.size)
    if nseg <= 0:
        return out, oe, np.zeros(idx.size, dtype=np.int32)
    dx = _native.device_upload(x, dev)
    ctx.dev_call("pai_segment_dot_dev", words.ptr, ex.ptr, N, idx.ctypes.data, off.ctypes.data, nseg,
                 _native.scalar_dtype(x), dx.ptr, out.ptr, oe.ptr, st.ptr)
    return out, oe, st.download(np.int32, idx.size)


def histogram_resident_args(N: int, bins, n_bins, node, n_nodes):
    """histogram_args when bins or node is a DeviceArray: what the host can check of a resident operand is its dtype and
    its shape (uint8 / uint16 C-contiguous [N, F]; int32 [N]); its values are the kernel's business (a node id outside
    [0, n_nodes) and a bin id >= n_bins put the sample in no cell). A host operand is checked as ever."""
    if isinstance(node, DeviceArray):
        if node.dtype != np.int32:
            raise TypeError(f"histogram: a device node array must be int32, not {node.dtype}")
        if node.shape != (N,):
            raise ValueError(f"histogram: node must have shape ({N},), not {node.shape}")
    if not isinstance(bins, DeviceArray):     # host bins with resident node ids: a stand-in node of the right shape
        b, _, shape = histogram_args(N, bins, n_bins, np.zeros(N, dtype=np.int32), n_nodes)
        return b, node, shape
    if bins.dtype not in (np.uint8, np.uint16):
        raise TypeError("histogram: bins must be uint8 or uint16")
    if bins.ndim != 2 or bins.shape[0] != N or bins.shape[1] == 0:
        raise ValueError(f"histogram: bins must have shape ({N}, F) with F >= 1, not {bins.shape}")
    # the scalar rules of histogram_args, on a one-row host stand-in of the same dtype and width
    one = np.zeros((1, bins.shape[1]), dtype=bins.dtype)
    host_node = node if not isinstance(node, DeviceArray) else np.zeros(N, dtype=np.int32)
    if host_node is not None:
        host_node = np.asarray(host_node)
        if host_node.dtype.kind in "iu" and host_node.shape != (N,):
            raise ValueError(f"histogram: node must have shape ({N},), not {host_node.shape}")
        _, nd, shape = histogram_args(1, one, n_bins, host_node[:1], n_nodes)
        if not isinstance(node, DeviceArray):
            node = np.clip(host_node, -1, int(n_nodes)).astype(np.int32)
    else:
        _, _, shape = histogram_args(1, one, n_bins, None, n_nodes)
    if N * bins.shape[1] >= 1 << 31:
        raise ValueError("histogram: bins must hold fewer than 2^31 entries")
    return bins, node, shape


def histogram_dev(pk, words: DeviceWords, exps, bins, n_bins: int, node, n_nodes: int):
    """pai_histogram_dev over the checked arguments of cipher_buffer.histogram_args: (words [cells, W], exponents,
    counts int64 on the host). Only the bins and the node ids go up, and not even those when they are DeviceArrays."""
    (N, W), dev = words.shape, words.device
    for a in (bins, node):
        if isinstance(a, DeviceArray) and a.device != dev:
            raise ValueError(f"the buffer lives on device {dev}, the operand on device {a.device}")
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    if not isinstance(bins, DeviceArray):
        bins = np.ascontiguousarray(bins)
    F = bins.shape[1]
    cells = int(n_nodes) * F * int(n_bins)
    db = bins.mem if isinstance(bins, DeviceArray) else _native.device_upload(bins, dev)
    if isinstance(node, DeviceArray):
        dn = node.mem
    else:
        dn = _native.device_upload(np.ascontiguousarray(node, dtype=np.int32), dev) if node is not None else None
    out, oe, cnt = DeviceWords.empty(cells, W, dev), _i32(dev, cells), _native.DeviceMem(cells * 8, dev)
    ctx.dev_call("pai_histogram_dev", words.ptr, ex.ptr, N,
                 _native.PAI_BIN_U16 if bins.dtype.itemsize == 2 else _native.PAI_BIN_U8, db.ptr, F, F,
                 dn.ptr if dn is not None else None, int(n_nodes), int(n_bins), out.ptr, oe.ptr, cnt.ptr)
    return out, oe, cnt.download(np.int64, cells)


def histogram_sparse_dev(pk, words: DeviceWords, exps, indptr, indices, data, zs, node, shape):
    """pai_histogram_sparse_dev over the checked arguments of cipher_buffer.histogram_sparse_args."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    nodes, F, B = shape
    cells = nodes * F * B
    up = lambda a, dt: _native.device_upload(np.ascontiguousarray(a, dtype=dt), dev)     # noqa: E731
    d_ptr, d_idx, d_dat, d_zs = up(indptr, np.int64), up(indices, np.int32), up(data, data.dtype), up(zs, np.int32)
    dn = up(node, np.int32) if node is not None else None
    out, oe, cnt = DeviceWords.empty(cells, W, dev), _i32(dev, cells), _native.DeviceMem(cells * 8, dev)
    ctx.dev_call("pai_histogram_sparse_dev", words.ptr, ex.ptr, N, d_ptr.ptr, d_idx.ptr,
                 _native.PAI_BIN_U16 if data.dtype.itemsize == 2 else _native.PAI_BIN_U8, d_dat.ptr, F, d_zs.ptr,
                 dn.ptr if dn is not None else None, nodes, B, out.ptr, oe.ptr, cnt.ptr)
    return out, oe, cnt.download(np.int64, cells)


def cumsum_dev(pk, words: DeviceWords, exps, outer: int, L: int, inner: int, reverse: bool = False):
    """pai_cumsum_dev: (words, exponents); launches only, nothing crosses PCIe."""
    (N, W), dev = words.shape, words.device
    if N != outer * L * inner:
        raise ValueError("cumsum: outer * L * inner must be the number of ciphertexts")
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    out, oe = DeviceWords.empty(N, W, dev), _i32(dev, N)
    ctx.dev_call("pai_cumsum_dev", words.ptr, ex.ptr, outer, L, inner,
                 _native.PAI_SCAN_REVERSE if reverse else 0, out.ptr, oe.ptr)
    return out, oe


def obfuscate_dev(pk, words: DeviceWords) -> DeviceWords:
    """c_i * r_i^n mod n^2 into a fresh block (pai_obfuscate_dev), by obfuscator.apply_obfuscation_array's rules:
    obfuscators prepared ahead of time when they cover the whole array, a fresh device-CSPRNG r per element otherwise."""
    from . import obfuscator_pool
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    out = DeviceWords.empty(N, W, dev)
    with obfuscator_pool.lock:
        pooled = obfuscator_pool.device_pool(pk, N)
        if pooled is not None:
            pooled.dev_call("pai_obfuscate_dev", words.ptr, N, _native.PAI_OBF_POOL, None, 0, 0, bytes(32), 0, out.ptr)
            return out
    ctx.dev_call("pai_obfuscate_dev", words.ptr, N, _native.PAI_OBF_RNG, None, 0, 0, os.urandom(32), 0, out.ptr)
    return out


def take_dev(pk, words: DeviceWords, exps, idx: np.ndarray):
    """pai_take_dev: (words [M, W], exponents [M]) of the rows idx names (host int64; -1: ciphertext 1, EMPTY_EXP)."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    out, oe = DeviceWords.empty(idx.size, W, dev), _i32(dev, idx.size)
    ctx.take_dev(words.ptr, ex.ptr, N, idx, out.ptr, oe.ptr)
    return out, oe


def upload_checked(pk, words: np.ndarray, device: int, message: str) -> DeviceWords:
    """Received words -> the device, range-checked there (pai_check_below_dev): ValueError(message) for a row >= n^2."""
    ctx = context_on(pk, device)
    dw = DeviceWords.from_host(words, device)
    if dw.shape[0] and ctx.check_below_dev(dw.ptr, dw.shape[0]) >= 0:
        raise ValueError(message)
    return dw


def pack_dev(pk, words: DeviceWords, exps, layout):
    """pai_pack_ciphertexts_dev: (packed words [ceil(N / slots), W], statuses [N] on the host)."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    ex = _exp_mem(exps, N, dev)
    lay = _native.pack_layout(layout)
    out, st = DeviceWords.empty(-(-N // lay.slots), W, dev), _i32(dev, N)
    if N:
        ctx.dev_call("pai_pack_ciphertexts_dev", words.ptr, ex.ptr, N, ctypes.byref(lay), out.ptr,
                     st.ptr)
    return out, st.download(np.int32, N)


def repack_dev(pk, words: DeviceWords, layout, group: int) -> DeviceWords:
    """pai_repack_dev: packed words [N, W] under `layout`, `group` at a time -> [ceil(N / group), W]."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev)
    lay, group = _native.pack_layout(layout), int(group)
    out = DeviceWords.empty(-(-N // group), W, dev)
    if N:
        ctx.dev_call("pai_repack_dev", words.ptr, N, ctypes.byref(lay), group, out.ptr)
    return out


def decrypt_dev(pk, private_key, words: DeviceWords, exps, want_raw: bool = False):
    """pai_decrypt_dev: (val float64, mant int64, statuses, raw words or None) on the host; no ciphertext word comes
    back."""
    (N, W), dev = words.shape, words.device
    ctx = context_on(pk, dev, private_key)
    ex = _exp_mem(exps, N, dev)
    val, mant, st = _native.DeviceMem(N * 8, dev), _native.DeviceMem(N * 8, dev), _i32(dev, N)
    raw = _native.DeviceMem(N * ctx.pt_words * 4, dev) if want_raw else None
    ctx.dev_call("pai_decrypt_dev", words.ptr, ex.ptr, N, val.ptr, mant.ptr, st.ptr,
                 raw.ptr if raw is not None else None)
    return (val.download(np.float64, N), mant.download(np.int64, N), st.download(np.int32, N),
            raw.download(np.uint32, N * ctx.pt_words).reshape(N, ctx.pt_words) if raw is not None else None)


def decrypt_packed_dev(pk, private_key, words: DeviceWords, layout, N: int):
    """pai_decrypt_packed_dev: (val float64 [N], mant int64 [N], statuses [N]) on the host."""
    dev, N = words.device, int(N)
    ctx = context_on(pk, dev, private_key)
    lay = _native.pack_layout(layout)
    val, mant, st = _native.DeviceMem(N * 8, dev), _native.DeviceMem(N * 8, dev), _i32(dev, N)
    ctx.dev_call("pai_decrypt_packed_dev", words.ptr, ctypes.byref(lay), N, val.ptr, mant.ptr, st.ptr)
    return val.download(np.float64, N), mant.download(np.int64, N), st.download(np.int32, N)


def encrypt_dev(pk, x: np.ndarray, exp_mode: int, fixed_exp: int):
    """pai_encrypt_dev of a float32 / float64 / int64 array under a fresh device-CSPRNG r (or obfuscators prepared ahead
    of time, when they cover the array): (words, exponents, statuses on the host). Only the plaintexts go up."""
    from . import _runtime, obfuscator_pool
    need_gpu()
    ctx = _runtime.context(pk)
    dev, W, N = ctx.device, ctx.ct_words, x.size
    dx = _native.device_upload(x, dev)
    out, oe, st = DeviceWords.empty(N, W, dev), _i32(dev, N), _i32(dev, N)
    args = (dx.ptr, N, exp_mode, fixed_exp)
    with obfuscator_pool.lock:
        pooled = obfuscator_pool.device_pool(pk, N)
        if pooled is not None:
            pooled.dev_call("pai_encrypt_dev", _native.scalar_dtype(x), *args, _native.PAI_OBF_POOL, None, 0, 0, bytes(32),
                            0, out.ptr, oe.ptr, st.ptr)
    if pooled is None:
        ctx.dev_call("pai_encrypt_dev", _native.scalar_dtype(x), *args, _native.PAI_OBF_RNG, None, 0, 0, os.urandom(32), 0,
                     out.ptr, oe.ptr, st.ptr)
    return out, oe, st.download(np.int32, N)


# ---------------------------------------------------------------------- the buffer
class DeviceCiphertextBuffer(BufferOps):
    """public_key, shape, size and obfuscated (a host uint8 array) as in CiphertextBuffer; the words (`words`, a
    DeviceWords) and the exponents live on `device`. `.exps` downloads the exponents once and caches them."""
    __slots__ = ("public_key", "words", "obfuscated", "shape", "_ex", "_exps", "__weakref__")

    def __init__(self, public_key, words: DeviceWords, exps, obfuscated=None, shape=None):
        """exps: a DeviceMem of N int32, or host exponents (uploaded, and kept as the cache)."""
        N, W = words.shape
        if W != ct_words(public_key):
            raise ValueError(f"ciphertext words {words.shape} do not match ({N}, {ct_words(public_key)}) for this key")
        self.public_key, self.words = public_key, words
        if isinstance(exps, _native.DeviceMem):
            if exps.nbytes < N * 4 or exps.device != words.device:
                raise ValueError("the exponents do not match the words")
            self._ex, self._exps = exps, None
        else:
            self._exps = np.ascontiguousarray(exps, dtype=np.int32).reshape(-1).copy()
            if self._exps.size != N:
                raise ValueError("the exponents do not match the words")
            self._ex = _native.device_upload(self._exps, words.device)
        if obfuscated is None:
            obfuscated = np.zeros(N, dtype=np.uint8)
        self.obfuscated = np.broadcast_to(np.asarray(obfuscated, dtype=np.uint8), (N,)).copy()
        self.shape = tuple(shape) if shape is not None else (N,)
        if int(np.prod(self.shape)) != N:
            raise ValueError("shape does not match the number of ciphertexts")

    # ---------------------------------------------------------------- conversions
    @classmethod
    def from_host(cls, buf: CiphertextBuffer) -> "DeviceCiphertextBuffer":
        from . import _runtime
        need_gpu()
        dev = _runtime.context(buf.public_key).device
        return cls(buf.public_key, DeviceWords.from_host(buf.words, dev), buf.exps, buf.obfuscated, buf.shape)

    @classmethod
    def from_pointers(cls, public_key, ct_ptr: int, exp_ptr: int, N: int, shape=None, owner=None, obfuscated=None,
                      device: Optional[int] = None) -> "DeviceCiphertextBuffer":
        """Wrap device memory somebody else owns, without a copy: ct_ptr names N * W uint32 words, exp_ptr N int32
        exponents (a torch tensor's data_ptr()). `owner` is kept alive as long as the buffer; nothing is freed."""
        from . import _runtime
        need_gpu()
        dev = _runtime.device_index() if device is None else int(device)
        N, W = int(N), ct_words(public_key)
        words = DeviceWords(_native.DeviceMem.wrap(ct_ptr, N * W * 4, dev, owner), N, W)
        return cls(public_key, words, _native.DeviceMem.wrap(exp_ptr, N * 4, dev, owner), obfuscated, shape)

    def to_host(self) -> CiphertextBuffer:
        """One download of the words (and of the exponents unless cached)."""
        return CiphertextBuffer(self.public_key, self.words.to_host(), self.exps, self.obfuscated, self.shape)

    def to_device(self) -> "DeviceCiphertextBuffer":
        return self

    def to_array(self):
        return self.to_host().to_array()

    def to_wire(self, be_secure: bool = False) -> bytes:
        """be_secure=True: apply_obfuscation() first. The bytes of CiphertextBuffer.to_wire, from one download."""
        from .cipher_array import _wire_bytes
        if be_secure:
            self.apply_obfuscation()
        return _wire_bytes(self.public_key.n, self.shape, self.exps, self.obfuscated, self.words.to_host())

    def data_ptr(self) -> int:
        return self.words.ptr

    def exps_ptr(self) -> int:
        return self._ex.ptr

    @property
    def device(self) -> int:
        return self.words.device

    @property
    def size(self) -> int:
        return self.words.shape[0]

    @property
    def nbytes(self) -> int:
        """Device bytes of the words and the exponents."""
        N, W = self.words.shape
        return N * W * 4 + N * 4

    @property
    def exps(self) -> np.ndarray:
        if self._exps is None:
            self._exps = self._ex.download(np.int32, self.size)
        return self._exps

    def release(self) -> None:
        """Free the device blocks now (after the device's queued work). Views made by reshape() end with them."""
        self.words.mem.free()
        self._ex.free()

    def __repr__(self) -> str:
        return (f"DeviceCiphertextBuffer(shape={self.shape}, key_bits={self.public_key.n.bit_length()}, "
                f"device={self.device})")

    def reshape(self, *shape) -> "DeviceCiphertextBuffer":
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        shape = tuple(np.empty(self.size, dtype=np.uint8).reshape(shape).shape)
        out = DeviceCiphertextBuffer(self.public_key, self.words, self._ex, self.obfuscated, shape)
        out._exps = self._exps
        return out

    def _ctx(self):
        return context_on(self.public_key, self.device)

    def _like(self, words: DeviceWords, exps, obfuscated=0, shape=None) -> "DeviceCiphertextBuffer":
        return DeviceCiphertextBuffer(self.public_key, words, exps, obfuscated, shape or self.shape)

    def _coerce(self, other) -> Optional["DeviceCiphertextBuffer"]:
        if isinstance(other, np.ndarray) and other.dtype == object:
            other = CiphertextBuffer.from_array(other)
        if not isinstance(other, (CiphertextBuffer, DeviceCiphertextBuffer)):
            return None
        if other.public_key != self.public_key:
            raise ValueError("add two numbers have different public key!")    # encrypted_number.py:169-170
        if other.shape != self.shape:
            raise ValueError(f"shapes {self.shape} and {other.shape} differ")
        if isinstance(other, CiphertextBuffer):
            self._ctx()
            return DeviceCiphertextBuffer(self.public_key, DeviceWords.from_host(other.words, self.device), other.exps,
                                          other.obfuscated, other.shape)
        if other.device != self.device:
            raise ValueError(f"buffers on devices {self.device} and {other.device}")
        return other

    # ---------------------------------------------------------------- operators (GPU, *_dev entry points only)
    def _add_plain(self, y):
        out, oe, st = add_plain_dev(self.public_key, self.words, self._ex, _plain(y, self.size))
        if np.any(st):
            # values the device flags (float overflow, |M| near max_int): the host class's operator as a whole, which
            # raises the reference's exception where the reference does
            return self.to_host()._add_plain(y).to_device()
        return self._like(out, oe)

    def __mul__(self, y):
        if isinstance(y, (PaillierEncryptedNumber, CiphertextBuffer, DeviceCiphertextBuffer)):
            raise ValueError("PaillierEncryptedNumber * PaillierEncryptedNumber is not allowed.")
        out, oe, st = mul_dev(self.public_key, self.words, self._ex, _plain(y, self.size))
        if np.any(st):
            return (self.to_host() * y).to_device()
        return self._like(out, oe)

    def segment_dot(self, index, seg_off, weights) -> "DeviceCiphertextBuffer":
        """CiphertextBuffer.segment_dot on the device (pai_segment_dot_dev)."""
        idx, off, w = segment_dot_args(self.size, index, seg_off, weights)
        out, oe, st = segment_dot_dev(self.public_key, self.words, self._ex, idx, off, w)
        bad = np.flatnonzero(st)
        if bad.size:
            t = int(bad[0])
            raise ValueError(f"segment_dot: weight {w[t]!r} at index {t} does not encode")
        nseg = off.size - 1
        e = np.where(np.diff(off) == 0, 0, oe.download(np.int32, nseg)).astype(np.int32)
        return self._like(out, e, 0, (nseg,))

    def _dense_dot(self, m: int, xs: np.ndarray, d: int, shape):
        out, oe = matmul_dev(self.public_key, self.words, self._ex, m, self.shape[-1], xs, d)
        return self._like(out, oe, 0, shape)

    def _gather(self, idx: np.ndarray, shape):
        out, oe = take_dev(self.public_key, self.words, self._ex, idx)
        return DeviceCiphertextBuffer(self.public_key, out, oe, self.obfuscated[idx], shape)

    def _take_resident(self, idx: DeviceArray) -> "DeviceCiphertextBuffer":
        if idx.dtype != np.int64:
            raise TypeError(f"take: a device index must be int64, not {idx.dtype}")
        out, oe, bad = take_idx_dev(self.public_key, self.words, self._ex, idx)
        if bad >= 0:
            raise IndexError(f"take: the index at position {bad} is out of bounds for {self.size} ciphertexts")
        return DeviceCiphertextBuffer(self.public_key, out, oe, 1 if bool(np.all(self.obfuscated)) else 0, idx.shape)

    def take(self, indices, axis=None):
        """np.take over the ciphertexts. An int64 DeviceArray names FLAT positions in [0, size) (axis must be None): the
        result has the index's shape and comes from one pai_take_idx_dev call that reads the index where it is; the 16
        bytes of the device-side check come back, and IndexError names the first bad position. The obfuscation flags are a
        host array and the index is not on the host, so the result is flagged obfuscated only when EVERY flag of this
        buffer is set, and unflagged otherwise: the safe side, at most one re-randomisation more."""
        if isinstance(indices, DeviceArray):
            if axis is not None:
                raise ValueError("take: a device index names flat positions (axis=None)")
            return self._take_resident(indices)
        return super().take(indices, axis)

    def __getitem__(self, key):
        """BufferOps.__getitem__; an int64 DeviceArray as in take()."""
        if isinstance(key, DeviceArray):
            return self._take_resident(key)
        return super().__getitem__(key)

    def segment_sum(self, index, seg_off) -> "DeviceCiphertextBuffer":
        """Per-segment sums: segment s is the sum of the ciphertexts at the flat positions index[seg_off[s] :
        seg_off[s + 1]] (repeats allowed), shape (nseg,); each sum is the reference's __add__ chain, an empty segment
        ciphertext 1 at exponent 0. Two numpy lists run as pai_segment_add_dev. When either is an int64 DeviceArray both
        are read on the device (pai_segment_add_idx_dev; a numpy one is uploaded for the call): nothing waits on the host
        but the 16 bytes of the device-side check, which raise what the host check raises. Not obfuscated."""
        idx = _index_operand("segment_sum", index, "index")
        off = _index_operand("segment_sum", seg_off, "seg_off")
        if idx.ndim != 1 or off.ndim != 1:
            raise ValueError("segment_sum: index and seg_off must be one-dimensional")
        if off.size < 1:
            raise ValueError("segment_sum: seg_off must start at 0 and must not decrease")
        nseg = off.size - 1
        if not isinstance(idx, DeviceArray) and not isinstance(off, DeviceArray):
            if off[0] != 0 or np.any(np.diff(off) < 0):
                raise ValueError("segment_sum: seg_off must start at 0 and must not decrease")
            if off[-1] != idx.size:
                raise ValueError(f"segment_sum: {idx.size} indices, seg_off ends at {int(off[-1])}")
            if idx.size and (idx.min() < 0 or idx.max() >= self.size):
                raise IndexError(f"segment_sum: index out of range for {self.size} ciphertexts")
            out, oe = segment_add_dev(self.public_key, self.words, self._ex, idx, off)
        else:
            self._ctx()
            d_idx = idx if isinstance(idx, DeviceArray) else device_array(idx, self.device)
            d_off = off if isinstance(off, DeviceArray) else device_array(off, self.device)
            out, oe, (bad_idx, bad_off) = segment_add_idx_dev(self.public_key, self.words, self._ex, d_idx, d_off)
            if bad_off >= 0:          # the error path may look: the offsets come down for the host check's message
                h = d_off.to_host()
                if h[0] != 0 or np.any(np.diff(h) < 0):
                    raise ValueError("segment_sum: seg_off must start at 0 and must not decrease")
                raise ValueError(f"segment_sum: {d_idx.size} indices, seg_off ends at {int(h[-1])}")
            if bad_idx >= 0:
                raise IndexError(f"segment_sum: index out of range for {self.size} ciphertexts")
        e = oe.download(np.int32, nseg)
        return self._like(out, np.where(e == EMPTY_EXP, 0, e).astype(np.int32), 0, (nseg,))

    def histogram(self, bins, n_bins: int, node=None, n_nodes: int = 1, default_bin=0):
        """CiphertextBuffer.histogram on the device (pai_histogram_dev, pai_histogram_sparse_dev): (DeviceCiphertextBuffer
        of shape (n_nodes, F, n_bins), int64 counts on the host). The empty cells' exponents are set to 0 on the
        exponents alone. Dense bins (uint8 / uint16, C-contiguous [N, F]) and node (int32 [N]) may be DeviceArrays: their
        pointers are passed through and nothing is uploaded for them, so a training run uploads its bins once. Sparse
        bins stay host operands."""
        csr = None if isinstance(bins, DeviceArray) else sparse_csr(bins)
        if csr is not None:
            if isinstance(node, DeviceArray):
                raise TypeError("histogram: sparse bins take host node ids")
            *args, shape = histogram_sparse_args(self.size, csr, n_bins, node, n_nodes, default_bin)
            out, oe, cnt = histogram_sparse_dev(self.public_key, self.words, self._ex, *args, shape)
        elif isinstance(bins, DeviceArray) or isinstance(node, DeviceArray):
            b, nd, shape = histogram_resident_args(self.size, bins, n_bins, node, n_nodes)
            out, oe, cnt = histogram_dev(self.public_key, self.words, self._ex, b, int(n_bins), nd, int(n_nodes))
        else:
            b, nd, shape = histogram_args(self.size, bins, n_bins, node, n_nodes)
            out, oe, cnt = histogram_dev(self.public_key, self.words, self._ex, b, int(n_bins), nd, int(n_nodes))
        e = np.where(cnt == 0, 0, oe.download(np.int32, cnt.size)).astype(np.int32)
        return self._like(out, e, 0, shape), cnt.reshape(shape)

    def cumsum(self, axis: int = -1, reverse: bool = False) -> "DeviceCiphertextBuffer":
        """CiphertextBuffer.cumsum on the device (pai_cumsum_dev): launches only."""
        outer, L, inner = axis_split(self.shape, axis)
        out, oe = cumsum_dev(self.public_key, self.words, self._ex, outer, L, inner, bool(reverse))
        return self._like(out, oe)

    def sum(self, axis=None) -> "DeviceCiphertextBuffer":
        """CiphertextBuffer.sum on the device (pai_segment_add_dev over index lists built from the shape)."""
        if axis is None:
            outer, L, inner, shape = 1, self.size, 1, (1,)
        else:
            outer, L, inner = axis_split(self.shape, axis)
            ax = axis % len(self.shape)
            shape = self.shape[:ax] + self.shape[ax + 1:] or (1,)
        idx = np.arange(outer * L * inner, dtype=np.int64).reshape(outer, L, inner).transpose(0, 2, 1).reshape(-1)
        off = np.arange(outer * inner + 1, dtype=np.int64) * L
        out, oe = segment_add_dev(self.public_key, self.words, self._ex, idx, off)
        e = oe.download(np.int32, off.size - 1)
        return self._like(out, np.where(e == EMPTY_EXP, 0, e).astype(np.int32), 0, shape)

    def apply_obfuscation(self) -> "DeviceCiphertextBuffer":
        """Re-randomise on the device (pai_obfuscate_dev) every ciphertext whose flag is not set, and set the flags.
        Flagged elements keep their bits; a second call makes no GPU call. Returns self."""
        todo = np.flatnonzero(self.obfuscated == 0)
        if todo.size == 0:
            return self
        pk, (N, W) = self.public_key, self.words.shape
        if todo.size == N:
            self.words = obfuscate_dev(pk, self.words)
        else:
            part, _ = take_dev(pk, self.words, self._ex, todo)
            fresh = obfuscate_dev(pk, part)
            both = DeviceWords.empty(N + todo.size, W, self.device)          # [the buffer | its re-randomised rows]
            both.mem.copy_from(self.words.mem, N * W * 4)
            both.mem.copy_from(fresh.mem, todo.size * W * 4, offset=N * W * 4)
            pick = np.arange(N, dtype=np.int64)
            pick[todo] = N + np.arange(todo.size, dtype=np.int64)
            self.words, _ = take_dev(pk, both, np.zeros(N + todo.size, dtype=np.int32), pick)
        self.obfuscated[todo] = 1
        return self

    def pack(self, layout, max_abs):
        """Fold these ciphertexts into a device-resident PackedCiphertextBuffer (pai_pack_ciphertexts_dev)."""
        from .packed_buffer import pack_ciphertexts
        return pack_ciphertexts(self, layout, max_abs)


def _as_device(b, like: DeviceCiphertextBuffer) -> DeviceCiphertextBuffer:
    if isinstance(b, DeviceCiphertextBuffer):
        return b
    if not isinstance(b, CiphertextBuffer):
        raise TypeError(f"unsupported operand {type(b)}")
    return DeviceCiphertextBuffer(b.public_key, DeviceWords.from_host(b.words, like.device), b.exps, b.obfuscated, b.shape)


def add_device_buffers(bufs: Sequence) -> DeviceCiphertextBuffer:
    """cipher_buffer.add_buffers when an operand lives on the device: ONE k-way pai_add_dev; host operands are
    uploaded for the call."""
    a = next(b for b in bufs if isinstance(b, DeviceCiphertextBuffer))
    ops = [a._coerce(b) if b is not a else a for b in bufs]
    if any(o is None for o in ops):
        raise TypeError("add_buffers: unsupported operand")
    if len(ops) == 1:
        return a
    out, oe = add_dev(a.public_key, [o.words for o in ops], [o._ex for o in ops])
    return a._like(out, oe)


def stack_device_buffers(bufs: Sequence) -> DeviceCiphertextBuffer:
    """The operands one after the other as one flat device buffer (device-to-device copies; cipher_buffer.concatenate
    picks its result out of it with one pai_take_dev)."""
    a = next(b for b in bufs if isinstance(b, DeviceCiphertextBuffer))
    a._ctx()
    ops = [_as_device(b, a) for b in bufs]
    for o in ops:
        if o.device != a.device:
            raise ValueError(f"buffers on devices {a.device} and {o.device}")
    W, total = a.words.shape[1], sum(o.size for o in ops)
    words, ex = DeviceWords.empty(total, W, a.device), _i32(a.device, total)
    at = 0
    for o in ops:
        words.mem.copy_from(o.words.mem, o.size * W * 4, offset=at * W * 4)
        ex.copy_from(o._ex, o.size * 4, offset=at * 4)
        at += o.size
    return DeviceCiphertextBuffer(a.public_key, words, ex, np.concatenate([o.obfuscated for o in ops]))
