"""CiphertextBuffer: ciphertext arrays in the packed device format, with no Python object per element.

A PaillierArray (cipher_array.py) is an object ndarray so that every reference caller keeps working; the
price is one PaillierEncryptedNumber and one Python int per element (~1 us each to build).
A party that only forwards, sums or scales ciphertexts -- the HE_SA_FT coordinator summing the parties'
gradients (he_sa_ft/train.py:64-71), a relay between two ionic_bond peers -- never needs those objects.
CiphertextBuffer keeps the words ([N, W] little-endian uint32), the exponents and the obfuscation flags
as numpy arrays, and runs the array operators straight on the GPU:

    buf = from_wire(received_bytes, lazy=True)      # no objects: validated words + exponents
    total = add_buffers([buf, other, third])        # ONE k-way k_add launch (encrypted_number.py:166-185)
    scaled = total * 0.5                            # ONE k_mul launch (encrypted_number.py:86-113)
    send(scaled.to_wire())                          # same bulk format, straight from the words
    values = decryptor.decrypt(scaled)              # ONE decrypt launch (decryptor.py:91-112)

Results are bit-identical to the per-object operators (same kernels as PaillierArray's). Conversions:
CiphertextBuffer.from_array(PaillierArray or object ndarray), .to_array() -> PaillierArray,
PaillierEncryptor.encrypt_to_buffer(ndarray). buf[key], buf.take, buf.T and concatenate select like numpy.
.to_device() gives a DeviceCiphertextBuffer (device_buffer.py): the same operators with the words kept on the GPU
between calls.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .encrypted_number import PaillierEncryptedNumber


def need_gpu() -> None:
    from . import _runtime
    if not _runtime.gpu_available():
        raise RuntimeError("CiphertextBuffer operators need a GPU (use .to_array() for the host operators)")


def _on_device(x) -> bool:
    from .device_buffer import DeviceCiphertextBuffer
    return isinstance(x, DeviceCiphertextBuffer)


class BufferOps(object):
    """What CiphertextBuffer and DeviceCiphertextBuffer (device_buffer.py) share: the operators that are written in
    terms of other operators, and indexing. A subclass provides public_key, shape, size, _coerce, _add_plain, __mul__,
    segment_dot, _dense_dot and _gather."""
    __slots__ = ()

    def __len__(self) -> int:
        return self.shape[0] if self.shape else 1

    def _broadcast(self, number) -> "CiphertextBuffer":
        return CiphertextBuffer.from_array(np.full(self.shape, number, dtype=object))

    def __add__(self, other):
        if _on_device(other) and not _on_device(self):
            return NotImplemented                               # other.__radd__: the sum stays on the device
        b = self._coerce(other)
        if b is not None:
            return add_buffers([self, b])
        if isinstance(other, PaillierEncryptedNumber):
            return add_buffers([self, self._coerce(self._broadcast(other))])
        return self._add_plain(other)

    __radd__ = __add__

    def __sub__(self, other):
        # self + (other * -1), encrypted_number.py:74-75: an encrypted operand is scaled by -1 on the GPU
        # (k_mul with the batch inversion) and added by k_add; a plain one is negated and added as plain
        if _on_device(other) and not _on_device(self):
            return NotImplemented                               # other.__rsub__
        if isinstance(other, PaillierEncryptedNumber):
            other = self._broadcast(other)
        b = self._coerce(other)
        if b is not None:
            return add_buffers([self, b * -1])
        return self._add_plain(_plain(other, self.size) * -1)

    def __rsub__(self, other):
        if isinstance(other, PaillierEncryptedNumber):
            other = self._broadcast(other)
        b = self._coerce(other)
        if b is not None:
            return add_buffers([b, self * -1])
        return (self * -1)._add_plain(other)                    # other + (self * -1), encrypted_number.py:77-78

    def __rmul__(self, y):
        return self * y

    def __truediv__(self, s):
        return self * (1 / s)

    def _dot_sparse(self, csc):
        indptr, indices, data, (K, d) = csc
        if len(self.shape) not in (1, 2) or K != self.shape[-1]:
            raise ValueError(f"dot: shapes {self.shape} and {(K, d)} not aligned")
        m = self.shape[0] if len(self.shape) == 2 else 1
        idx, off, w = sparse_segments(indptr, indices, data, m, K, d)
        out = self.segment_dot(idx, off, w)
        return out.reshape((m, d) if len(self.shape) == 2 else (d,))

    def dot(self, b):
        """(K,) or (m, K) encrypted @ (K,) or (K, d) plain, numpy semantics (he_otp_lr_ft1/train.py:160). A sparse
        (K, d) matrix (anything that offers .tocsc()) runs as segment_dot over its stored entries, explicit zeros
        included: columns are the segments, row i of an (m, K) buffer offsets the indices by i K."""
        csc = sparse_csc(b)
        if csc is not None:
            return self._dot_sparse(csc)
        x = np.asarray(b)
        if len(self.shape) not in (1, 2) or x.ndim not in (1, 2) or x.shape[0] != self.shape[-1]:
            raise ValueError(f"dot: shapes {self.shape} and {x.shape} not aligned")
        from .cipher_array import _plain_array
        xs = _plain_array(x)
        if xs is None:
            raise TypeError(f"dot: unsupported operand dtype {x.dtype}")
        m = self.shape[0] if len(self.shape) == 2 else 1
        d = x.shape[1] if x.ndim == 2 else 1
        shape = tuple(([m] if len(self.shape) == 2 else []) + ([d] if x.ndim == 2 else []))
        return self._dense_dot(m, np.ascontiguousarray(xs).reshape(-1), d, shape if shape else (1,))

    def __matmul__(self, b):
        return self.dot(b)

    # ---------------------------------------------------------------- indexing (numpy semantics)
    def _positions(self) -> np.ndarray:
        return np.arange(self.size, dtype=np.int64).reshape(self.shape)

    def _select(self, idx) -> "CiphertextBuffer":
        idx = np.asarray(idx, dtype=np.int64)
        return self._gather(np.ascontiguousarray(idx).reshape(-1), idx.shape)

    def __getitem__(self, key):
        """buf[key] with numpy's rules (ints, slices, integer arrays, boolean masks, ... and None): the elements that
        np.arange(size).reshape(shape)[key] names, in that shape. One selected element is a buffer of shape (), not a
        scalar. The obfuscation flags travel with their elements."""
        return self._select(self._positions()[key])

    def take(self, indices, axis=None):
        """np.take(array, indices, axis) over the ciphertexts."""
        return self._select(np.take(self._positions(), indices, axis=axis))

    def transpose(self, *axes):
        """np.transpose over the ciphertexts (a copy: both buffer classes keep their elements C-contiguous)."""
        axes = axes[0] if len(axes) == 1 and (axes[0] is None or isinstance(axes[0], (tuple, list))) else (axes or None)
        return self._select(np.transpose(self._positions(), axes))

    @property
    def T(self):
        return self.transpose()


class CiphertextBuffer(BufferOps):
    __slots__ = ("public_key", "words", "exps", "obfuscated", "shape")

    def __init__(self, public_key, words: np.ndarray, exps: np.ndarray, obfuscated=None, shape=None):
        W = (2 * public_key.n.bit_length() + 31) // 32
        words = np.ascontiguousarray(words, dtype=np.uint32)
        exps = np.ascontiguousarray(exps, dtype=np.int32).reshape(-1)
        N = exps.size
        if words.shape != (N, W):
            raise ValueError(f"ciphertext words {words.shape} do not match ({N}, {W}) for this key")
        self.public_key = public_key
        self.words = words
        self.exps = exps
        if obfuscated is None:
            obfuscated = np.zeros(N, dtype=np.uint8)
        self.obfuscated = np.broadcast_to(np.asarray(obfuscated, dtype=np.uint8), (N,)).copy()
        self.shape = tuple(shape) if shape is not None else (N,)
        if int(np.prod(self.shape)) != N:
            raise ValueError("shape does not match the number of ciphertexts")

    # ---------------------------------------------------------------- conversions
    @classmethod
    def from_array(cls, arr) -> "CiphertextBuffer":
        """Pack a PaillierArray / object ndarray of PaillierEncryptedNumber (one public key)."""
        from .cipher_array import _encrypted_operand, pack
        A, pk = _encrypted_operand(arr)
        if A is None:
            raise TypeError("from_array needs a non-empty array of PaillierEncryptedNumber with one public key")
        words, exps, _ = pack(arr, pk)
        obf = np.fromiter((e._is_obfuscated() for e in A.reshape(-1)), dtype=np.uint8, count=A.size)
        return cls(pk, words, exps, obf, A.shape)

    def to_array(self):
        """PaillierArray of PaillierEncryptedNumber (materialises one object per element)."""
        from .cipher_array import materialize
        return materialize(self.public_key, self.words, self.exps, self.shape, obfuscated=self.obfuscated != 0)

    def apply_obfuscation(self) -> "CiphertextBuffer":
        """Re-randomise, in place and in ONE GPU call (pai_obfuscate), every ciphertext whose flag is not set, and
        set the flags: PaillierEncryptedNumber.apply_obfuscation (encrypted_number.py:58-63) per element, with no
        object built. Flagged elements keep their bits; a second call makes no GPU call. Returns self."""
        from .obfuscator import apply_obfuscation_array
        todo = np.flatnonzero(self.obfuscated == 0)
        if todo.size == 0:
            return self
        if todo.size == self.size:
            self.words = apply_obfuscation_array(self.words, self.public_key)
        else:
            words = self.words.copy()
            words[todo] = apply_obfuscation_array(self.words[todo], self.public_key)
            self.words = words
        self.obfuscated[todo] = 1
        return self

    def to_wire(self, be_secure: bool = False) -> bytes:
        """be_secure=True: apply_obfuscation() first, so every shipped flag is 1."""
        from .cipher_array import _wire_bytes
        if be_secure:
            self.apply_obfuscation()
        return _wire_bytes(self.public_key.n, self.shape, self.exps, self.obfuscated, self.words)

    def reshape(self, *shape) -> "CiphertextBuffer":
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        shape = tuple(np.empty(self.size, dtype=np.uint8).reshape(shape).shape)
        return CiphertextBuffer(self.public_key, self.words, self.exps, self.obfuscated, shape)

    @property
    def size(self) -> int:
        return self.exps.size

    def __repr__(self) -> str:
        return f"CiphertextBuffer(shape={self.shape}, key_bits={self.public_key.n.bit_length()})"

    def _ctx(self):
        from . import _runtime
        need_gpu()
        return _runtime.context(self.public_key)

    def _like(self, words, exps, obfuscated=0, shape=None) -> "CiphertextBuffer":
        return CiphertextBuffer(self.public_key, words, exps, obfuscated, shape or self.shape)

    def _coerce(self, other) -> Optional["CiphertextBuffer"]:
        if isinstance(other, CiphertextBuffer):
            b = other
        elif isinstance(other, np.ndarray) and other.dtype == object:
            b = CiphertextBuffer.from_array(other)
        else:
            return None
        if b.public_key != self.public_key:
            raise ValueError("add two numbers have different public key!")    # encrypted_number.py:169-170
        if b.shape != self.shape:
            raise ValueError(f"shapes {self.shape} and {b.shape} differ")
        return b

    # ---------------------------------------------------------------- operators (GPU)
    def _add_plain(self, y):
        x = _plain(y, self.size)
        out, oe, st = self._ctx().add_plain(self.words, self.exps, x)
        bad = np.flatnonzero(st)
        if bad.size:
            # values the device flags (float overflow, |M| near max_int): the per-element operator, which
            # raises the reference's exception where it does
            out = out.copy()
            oe = oe.copy()
            ints = _ints(self.words[bad])
            for j, i in enumerate(bad.tolist()):
                r = PaillierEncryptedNumber(self.public_key, ints[j], int(self.exps[i])) + _item(y, i)
                out[i] = _words(r.ciphertext(False), self.words.shape[1])
                oe[i] = r.exponent
        return self._like(out, oe)

    def __mul__(self, y):
        if isinstance(y, (PaillierEncryptedNumber, CiphertextBuffer)):
            raise ValueError("PaillierEncryptedNumber * PaillierEncryptedNumber is not allowed.")
        out, oe, _ = self._ctx().mul(self.words, self.exps, _plain(y, self.size))
        return self._like(out, oe)

    def segment_dot(self, index, seg_off, weights) -> "CiphertextBuffer":
        """Segmented weighted sums, shape (nseg,): out[s] = sum over t in [seg_off[s], seg_off[s+1]) of
        self[index[t]] * weights[t] (flat indices; pai_segment_dot, one call). Each term is the reference's __mul__, each
        sum its __add__ chain; a weight that does not encode raises ValueError naming its position. An empty segment
        is ciphertext 1 at exponent 0, an unobfuscated encryption of 0. Without a GPU the same runs on Python integers."""
        idx, off, w = segment_dot_args(self.size, index, seg_off, weights)
        out, oe = segment_dot_words(self.public_key, self.words, self.exps, idx, off, w)
        return self._like(out, oe, 0, (off.size - 1,))

    def _dense_dot(self, m: int, xs: np.ndarray, d: int, shape):
        out, oe = self._ctx().matmul(self.words, self.exps, m, self.shape[-1], xs, d)
        return self._like(out, oe, 0, shape)

    def _gather(self, idx: np.ndarray, shape):
        return CiphertextBuffer(self.public_key, self.words[idx], self.exps[idx], self.obfuscated[idx], shape)

    def to_device(self):
        """The same ciphertexts as a DeviceCiphertextBuffer (device_buffer.py): one upload; RuntimeError without a GPU."""
        from .device_buffer import DeviceCiphertextBuffer
        return DeviceCiphertextBuffer.from_host(self)

    def histogram(self, bins, n_bins: int, node=None, n_nodes: int = 1, default_bin=0):
        """Per-cell sums of these N ciphertexts (flat order) over the bin ids bins [N, F] (uint8 / uint16) and an optional
        node id per sample: (CiphertextBuffer of shape (n_nodes, F, n_bins), int64 counts of that shape), cell
        [v, f, b] = the sum of the samples with node == v and bins[:, f] == b, in ONE pai_histogram call with no index
        list. A node id outside [0, n_nodes) and a bin id >= n_bins put the sample in no cell (of that feature). Each
        sum is the reference's __add__ chain over the members; an empty cell is ciphertext 1 at exponent 0, an
        unobfuscated encryption of 0. Without a GPU the same runs on Python integers.
        Sparse bins (anything that offers .tocsr(); never densified, never re-routed to the dense call) take ONE
        pai_histogram_sparse call whose cost follows the stored entries: an entry that is not stored has bin
        default_bin (a scalar or one per feature, out of range: in no cell), and the default cell [v, f, default_bin[f]]
        is T_v - S: the node's total minus the feature's stored entries off the default bin, at the node's largest
        exponent (the dense call's plaintext; its bits too wherever a node's exponents are uniform)."""
        csr = sparse_csr(bins)
        if csr is not None:
            *args, shape = histogram_sparse_args(self.size, csr, n_bins, node, n_nodes, default_bin)
            out, oe, cnt = histogram_sparse_words(self.public_key, self.words, self.exps, *args, shape)
            oe = np.where(cnt == 0, 0, oe).astype(np.int32)
            return self._like(out, oe, 0, shape), cnt.reshape(shape)
        b, nd, shape = histogram_args(self.size, bins, n_bins, node, n_nodes)
        out, oe, cnt = histogram_words(self.public_key, self.words, self.exps, b, int(n_bins), nd, int(n_nodes))
        oe = np.where(cnt == 0, 0, oe).astype(np.int32)
        return self._like(out, oe, 0, shape), cnt.reshape(shape)

    def cumsum(self, axis: int = -1, reverse: bool = False) -> "CiphertextBuffer":
        """Running sums along `axis` (reverse: from the end), same shape, in ONE pai_cumsum call: element j is the
        reference's __add__ chain over the elements up to j (np.cumsum over PaillierEncryptedNumber), at the largest
        exponent of that prefix. An empty cell of a histogram (ciphertext 1, exponent 0) adds 0 like any other element.
        Not obfuscated. Without a GPU the same runs on Python integers."""
        outer, L, inner = axis_split(self.shape, axis)
        out, oe = cumsum_words(self.public_key, self.words, self.exps, outer, L, inner, bool(reverse))
        return self._like(out, oe)

    def sum(self, axis=None) -> "CiphertextBuffer":
        """Sum over `axis` (None: over everything, shape (1,)) in ONE pai_segment_add call over index lists built from
        the shape; each sum is the reference's __add__ chain. An empty reduction is ciphertext 1 at exponent 0, an
        unobfuscated encryption of 0. Without a GPU the same runs on Python integers."""
        if axis is None:
            outer, L, inner, shape = 1, self.size, 1, (1,)
        else:
            outer, L, inner = axis_split(self.shape, axis)
            ax = axis % len(self.shape)
            shape = self.shape[:ax] + self.shape[ax + 1:] or (1,)
        idx = np.arange(outer * L * inner, dtype=np.int64).reshape(outer, L, inner).transpose(0, 2, 1).reshape(-1)
        off = np.arange(outer * inner + 1, dtype=np.int64) * L
        out, oe = segment_add_words(self.public_key, self.words, self.exps, idx, off)
        oe = np.where(oe == EMPTY_EXP, 0, oe).astype(np.int32)
        return self._like(out, oe, 0, shape)

    def pack(self, layout, max_abs):
        """Fold these ciphertexts into a PackedCiphertextBuffer (packed_buffer.pack_ciphertexts)."""
        from .packed_buffer import pack_ciphertexts
        return pack_ciphertexts(self, layout, max_abs)


def add_buffers(bufs: Sequence[CiphertextBuffer]) -> CiphertextBuffer:
    """Element-wise sum of k buffers of one key and shape in ONE k-way add launch (the reference's
    left-to-right __add__ chain gives the same ciphertexts: each sum is the product of the operands
    aligned to the largest exponent)."""
    bufs = list(bufs)
    if not bufs:
        raise ValueError("add_buffers needs at least one buffer")
    if any(_on_device(b) for b in bufs):       # one device buffer keeps the sum on the device
        from .device_buffer import add_device_buffers
        return add_device_buffers(bufs)
    a = bufs[0]
    for b in bufs[1:]:
        a._coerce(b)
    if len(bufs) == 1:
        return a
    out, oe = a._ctx().add([b.words for b in bufs], [b.exps for b in bufs])
    return a._like(out, oe)


def concatenate(bufs: Sequence[CiphertextBuffer], axis: int = 0):
    """np.concatenate over buffers of one key: a CiphertextBuffer, or a DeviceCiphertextBuffer when any operand is one
    (device-to-device copies and one pai_take_dev; host operands are uploaded for the call)."""
    bufs = list(bufs)
    if not bufs:
        raise ValueError("need at least one buffer to concatenate")
    for b in bufs[1:]:
        if b.public_key != bufs[0].public_key:
            raise ValueError("add two numbers have different public key!")
    starts = np.cumsum([0] + [b.size for b in bufs[:-1]])
    idx = np.concatenate([b._positions() + int(o) for b, o in zip(bufs, starts)], axis=axis)
    if any(_on_device(b) for b in bufs):
        from .device_buffer import stack_device_buffers
        return stack_device_buffers(bufs)._select(idx)
    a = bufs[0]
    flat = CiphertextBuffer(a.public_key, np.concatenate([b.words for b in bufs]), np.concatenate([b.exps for b in bufs]),
                            np.concatenate([b.obfuscated for b in bufs]))
    return flat._select(idx)


def sparse_csc(b):
    """(indptr, indices, data, shape) of a 2-D sparse matrix in CSC form, for any object that offers .tocsc() (duck
    typing: scipy is not imported here); None for everything else."""
    if isinstance(b, np.ndarray) or not hasattr(b, "tocsc"):
        return None
    c = b.tocsc()
    shape = tuple(int(v) for v in c.shape)
    if len(shape) != 2:
        raise ValueError(f"dot: sparse operand of shape {shape} is not a matrix")
    indptr = np.asarray(c.indptr, dtype=np.int64).reshape(-1)
    indices = np.asarray(c.indices, dtype=np.int64).reshape(-1)
    data = np.asarray(c.data).reshape(-1)
    if indptr.size != shape[1] + 1 or indices.size != data.size:
        raise ValueError("dot: malformed CSC operand")
    return indptr, indices, data, shape


def sparse_segments(indptr, indices, data, m: int, K: int, d: int):
    """(index, seg_off, weights) of an (m, K) encrypted times (K, d) CSC product: segment i d + j is column j over the
    ciphertexts of row i."""
    nnz = indices.size
    if indices.size and (indices.min() < 0 or indices.max() >= K):
        raise ValueError("dot: sparse row index out of range")
    idx = (indices[None, :] + (np.arange(m, dtype=np.int64) * K)[:, None]).reshape(-1)
    off = (indptr[None, :-1] + (np.arange(m, dtype=np.int64) * nnz)[:, None]).reshape(-1)
    off = np.concatenate([off, [m * nnz]]).astype(np.int64)
    return idx, off, np.tile(data, m)


def segment_dot_args(N: int, index, seg_off, weights):
    """Checked (index int64 [nnz], seg_off int64 [nseg + 1], weights of a device dtype [nnz])."""
    from .cipher_array import _plain_array
    idx = np.asarray(index)
    off = np.asarray(seg_off)
    w = np.asarray(weights)
    if idx.ndim != 1 or off.ndim != 1 or w.ndim != 1:
        raise ValueError("segment_dot: index, seg_off and weights must be one-dimensional")
    if (idx.size and idx.dtype.kind not in "iu") or (off.dtype.kind not in "iu"):
        raise TypeError("segment_dot: index and seg_off must be integers")
    idx = idx.astype(np.int64)
    off = off.astype(np.int64)
    if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("segment_dot: seg_off must start at 0 and must not decrease")
    if off[-1] != idx.size or w.size != idx.size:
        raise ValueError(f"segment_dot: {idx.size} indices, {w.size} weights, seg_off ends at {int(off[-1])}")
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        raise IndexError(f"segment_dot: index out of range for {N} ciphertexts")
    x = _plain_array(w) if w.size else w.astype(np.float64)
    if x is None:
        raise TypeError(f"segment_dot: unsupported weight dtype {w.dtype}")
    return idx, off, np.ascontiguousarray(x)


def segment_dot_words(pk, words, exps, idx, off, w):
    """(words [nseg, W], exponents [nseg]) of the segmented weighted sums over checked arguments: pai_segment_dot on the
    GPU, the per-element operators on Python integers without one. Empty segments: ciphertext 1, exponent 0."""
    from . import _runtime
    nseg = off.size - 1
    W = words.shape[1]
    if _runtime.gpu_available():
        out, oe, st = _runtime.context(pk).segment_dot(words, exps, idx, off, w)
        bad = np.flatnonzero(st)
        if bad.size:
            t = int(bad[0])
            raise ValueError(f"segment_dot: weight {w[t]!r} at index {t} does not encode")
        oe = np.where(np.diff(off) == 0, 0, oe).astype(np.int32)
        return out, oe
    cts = _ints(words)
    vals, oe = [], []
    for s in range(nseg):
        acc = None
        for t in range(int(off[s]), int(off[s + 1])):
            i = int(idx[t])
            try:
                term = PaillierEncryptedNumber(pk, cts[i], int(exps[i])) * w[t]
            except (ValueError, OverflowError) as e:
                raise ValueError(f"segment_dot: weight {w[t]!r} at index {t} does not encode") from e
            acc = term if acc is None else acc + term
        vals.append(1 if acc is None else acc.ciphertext(False))
        oe.append(0 if acc is None else acc.exponent)
    return _runtime.ints_to_words(vals, W).reshape(nseg, W), np.array(oe, dtype=np.int32)


EMPTY_EXP = -(1 << 31)      # the exponent of an empty cell or segment (ciphertext 1)


def _device_words(words) -> bool:
    """True for a device holder (device_buffer.DeviceWords) in the place of numpy words: histogram_words,
    histogram_sparse_words and cumsum_words then run the *_dev entry points and return (DeviceWords, exponents as a
    device block[, counts on the host]), which is how both buffer classes and the packed buffer stay resident."""
    if isinstance(words, np.ndarray):
        return False
    from .device_buffer import DeviceWords
    return isinstance(words, DeviceWords)


def axis_split(shape, axis):
    """(outer, L, inner) of a C-contiguous array of `shape` scanned or reduced along `axis`."""
    if isinstance(axis, (bool, np.bool_)) or not isinstance(axis, (int, np.integer)):
        raise TypeError("axis must be an integer")
    nd = len(shape)
    if not -nd <= axis < nd:
        raise ValueError(f"axis {axis} is out of bounds for an array of dimension {nd}")
    ax = int(axis) % nd
    return int(np.prod(shape[:ax], dtype=np.int64)), int(shape[ax]), int(np.prod(shape[ax + 1:], dtype=np.int64))


def cumsum_words(pk, words, exps, outer: int, L: int, inner: int, reverse: bool = False):
    """(words [outer L inner, W], exponents) of the prefix sums along the middle axis: pai_cumsum on the GPU, products of
    Python integers without one. Entries with exponent EMPTY_EXP are skipped; a prefix of such entries only is
    ciphertext 1 with exponent EMPTY_EXP."""
    from . import _runtime
    if _device_words(words):
        from . import device_buffer
        return device_buffer.cumsum_dev(pk, words, exps, outer, L, inner, reverse)
    N, W = outer * L * inner, words.shape[1]
    if N != np.asarray(exps).size:
        raise ValueError("cumsum: outer * L * inner must be the number of ciphertexts")
    if N and _runtime.gpu_available():
        return _runtime.context(pk).cumsum(words, exps, outer, L, inner, reverse)
    cts, nsq = _ints(words), pk.nsquare
    ex = [int(e) for e in np.asarray(exps).reshape(-1)]
    vals, oe = [1] * N, [EMPTY_EXP] * N
    order = range(L - 1, -1, -1) if reverse else range(L)
    for o in range(outer):
        for i in range(inner):
            acc, E = 1, EMPTY_EXP
            for j in order:
                t = (o * L + j) * inner + i
                if ex[t] != EMPTY_EXP:
                    if E == EMPTY_EXP:
                        acc, E = cts[t], ex[t]
                    elif ex[t] > E:
                        acc, E = pow(acc, 16 ** (ex[t] - E), nsq) * cts[t] % nsq, ex[t]
                    else:
                        acc = acc * pow(cts[t], 16 ** (E - ex[t]), nsq) % nsq
                vals[t], oe[t] = acc, E
    return _runtime.ints_to_words(vals, W).reshape(N, W), np.array(oe, dtype=np.int32).reshape(N)


def segment_add_words(pk, words, exps, idx, off):
    """(words [nseg, W], exponents [nseg]) of the per-segment sums: pai_segment_add on the GPU, products of Python
    integers without one. Empty segments: ciphertext 1, exponent EMPTY_EXP."""
    from . import _runtime
    nseg, W = off.size - 1, words.shape[1]
    if nseg and _runtime.gpu_available():
        return _runtime.context(pk).segment_add(words, exps, idx, off)
    cts, nsq = _ints(words), pk.nsquare
    vals, oe = [], []
    for s in range(nseg):
        mem = [int(t) for t in idx[int(off[s]):int(off[s + 1])]]
        E = max((int(exps[t]) for t in mem), default=EMPTY_EXP)
        acc = 1
        for t in mem:
            acc = acc * pow(cts[t], 16 ** (E - int(exps[t])), nsq) % nsq
        vals.append(acc)
        oe.append(E)
    return _runtime.ints_to_words(vals, W).reshape(nseg, W), np.array(oe, dtype=np.int32).reshape(nseg)


def histogram_args(N: int, bins, n_bins, node, n_nodes):
    """Checked (bins uint8 / uint16 [N, F] with contiguous rows, node int32 [N] or None, (n_nodes, F, n_bins))."""
    if not isinstance(bins, np.ndarray) or bins.dtype not in (np.uint8, np.uint16):
        raise TypeError("histogram: bins must be a numpy array of uint8 or uint16")
    if bins.ndim != 2 or bins.shape[0] != N or bins.shape[1] == 0:
        raise ValueError(f"histogram: bins must have shape ({N}, F) with F >= 1, not {bins.shape}")
    isz = bins.dtype.itemsize
    F = bins.shape[1]
    if N > 1 and (bins.strides[1] != isz or bins.strides[0] % isz or bins.strides[0] < F * isz):
        raise ValueError("histogram: bins must be C-contiguous or row-strided (contiguous rows)")
    if isinstance(n_bins, (bool, np.bool_)) or not isinstance(n_bins, (int, np.integer)):
        raise TypeError("histogram: n_bins must be an integer")
    if not 1 <= int(n_bins) <= (256 if isz == 1 else 65536):
        raise ValueError(f"histogram: n_bins must be in 1 .. {256 if isz == 1 else 65536} for {bins.dtype} bins")
    if isinstance(n_nodes, (bool, np.bool_)) or not isinstance(n_nodes, (int, np.integer)):
        raise TypeError("histogram: n_nodes must be an integer")
    if int(n_nodes) < 1:
        raise ValueError("histogram: n_nodes must be at least 1")
    if node is None:
        if int(n_nodes) != 1:
            raise ValueError("histogram: n_nodes must be 1 without node ids")
    else:
        node = np.asarray(node)
        if node.dtype.kind not in "iu":
            raise TypeError("histogram: node must hold integers")
        if node.shape != (N,):
            raise ValueError(f"histogram: node must have shape ({N},), not {node.shape}")
        node = np.clip(node, -1, int(n_nodes)).astype(np.int32)       # out of range stays out of range
    if int(n_nodes) * F * int(n_bins) > 1 << 24:
        raise ValueError("histogram: more than 2^24 cells")
    if N * F >= 1 << 31:
        raise ValueError("histogram: bins must hold fewer than 2^31 entries")
    return bins, node, (int(n_nodes), F, int(n_bins))


def histogram_cells(bins, n_bins: int, node, n_nodes: int):
    """Host side of the cell rule: the flat cell (v F + f) n_bins + b of every (sample, feature) pair, -1 where the
    sample is in no cell of that feature; shape [N, F]."""
    N, F = bins.shape
    b = bins.astype(np.int64)
    v = np.zeros(N, dtype=np.int64) if node is None else node.astype(np.int64)
    ok = (b < n_bins) & ((v >= 0) & (v < n_nodes))[:, None]
    cell = (v[:, None] * F + np.arange(F, dtype=np.int64)[None, :]) * n_bins + b
    return np.where(ok, cell, -1)


def histogram_words(pk, words, exps, bins, n_bins: int, node, n_nodes: int):
    """(words [cells, W], exponents [cells], counts int64 [cells]) of the histogram over checked arguments: pai_histogram
    on the GPU, products of Python integers without one. Empty cells: ciphertext 1, exponent EMPTY_EXP."""
    from . import _runtime
    if _device_words(words):
        from . import device_buffer
        return device_buffer.histogram_dev(pk, words, exps, bins, n_bins, node, n_nodes)
    if _runtime.gpu_available():
        return _runtime.context(pk).histogram(words, exps, bins, n_bins, node, n_nodes)
    W = words.shape[1]
    cells = n_nodes * bins.shape[1] * n_bins
    cell = histogram_cells(bins, n_bins, node, n_nodes)
    cts, nsq = _ints(words), pk.nsquare
    E = np.full(cells, EMPTY_EXP, dtype=np.int64)
    ii, ff = np.nonzero(cell >= 0)
    np.maximum.at(E, cell[ii, ff], np.asarray(exps, dtype=np.int64)[ii])
    cnt = np.bincount(cell[ii, ff], minlength=cells).astype(np.int64)
    acc = [1] * cells
    for i, f in zip(ii.tolist(), ff.tolist()):
        s = int(cell[i, f])
        acc[s] = acc[s] * pow(cts[i], 16 ** (int(E[s]) - int(exps[i])), nsq) % nsq
    return _runtime.ints_to_words(acc, W).reshape(cells, W), E.astype(np.int32), cnt


def sparse_csr(b):
    """(indptr, indices, data, shape) of a 2-D sparse matrix in canonical CSR form, for any object that offers .tocsr()
    (duck typing: scipy is not imported here); None for everything else. Duplicates are summed and the indices sorted
    where the object offers sum_duplicates() / sort_indices(), on a copy when .tocsr() returned the operand itself."""
    if isinstance(b, np.ndarray) or not hasattr(b, "tocsr"):
        return None
    c = b.tocsr()
    if c is b and hasattr(c, "copy"):
        c = c.copy()
    for name in ("sum_duplicates", "sort_indices"):
        fn = getattr(c, name, None)
        if callable(fn):
            fn()
    shape = tuple(int(v) for v in c.shape)
    if len(shape) != 2:
        raise ValueError(f"histogram: sparse bins of shape {shape} are not a matrix")
    indptr = np.asarray(c.indptr).reshape(-1)
    indices = np.asarray(c.indices).reshape(-1)
    data = np.asarray(c.data).reshape(-1)
    if (indptr.size != shape[0] + 1 or indices.size != data.size or indptr.dtype.kind not in "iu"
            or (indices.size and indices.dtype.kind not in "iu")):
        raise ValueError("histogram: malformed CSR operand")
    return indptr.astype(np.int64), indices.astype(np.int64), data, shape


def histogram_sparse_args(N: int, csr, n_bins, node, n_nodes, default_bin):
    """Checked (indptr int64 [N + 1], indices int32 [nnz], data uint8 / uint16 [nnz], default bins int32 [F] with -1 for
    "in no cell", node int32 [N] or None, (n_nodes, F, n_bins)) of a histogram over the CSR bins of sparse_csr. Stored
    ids are cast to uint8 below 256 bins and to uint16 from there; an id >= n_bins (a missing value) becomes n_bins."""
    indptr, indices, data, (rows, F) = csr
    if rows != N or F == 0:
        raise ValueError(f"histogram: bins must have shape ({N}, F) with F >= 1, not {(rows, F)}")
    if isinstance(n_bins, (bool, np.bool_)) or not isinstance(n_bins, (int, np.integer)):
        raise TypeError("histogram: n_bins must be an integer")
    B = int(n_bins)
    if not 1 <= B <= 65536:
        raise ValueError("histogram: n_bins must be in 1 .. 65536")
    # (the dense rules for node and n_nodes, and the cell limit)
    _, node, shape = histogram_args(N, np.zeros((N, 1), dtype=np.uint16), 1, node, n_nodes)
    if shape[0] * F * B > 1 << 24:
        raise ValueError("histogram: more than 2^24 cells")
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != indices.size:
        raise ValueError("histogram: indptr must start at 0, must not decrease and must end at the stored entries")
    if indices.size >= 1 << 31:
        raise ValueError("histogram: bins must hold fewer than 2^31 stored entries")
    if indices.size and (indices.min() < 0 or indices.max() >= F):
        raise IndexError(f"histogram: feature index out of range for {F} features")
    if indices.size > 1:
        inner = np.ones(indices.size - 1, dtype=bool)
        ends = indptr[1:-1]
        inner[ends[(ends > 0) & (ends < indices.size)] - 1] = False        # pairs that straddle two rows
        if np.any((np.diff(indices) <= 0) & inner):
            raise ValueError("histogram: the feature indices of a row must be strictly increasing (sorted, no duplicates)")
    if data.dtype.kind == "f":
        if not np.all(np.isfinite(data)) or np.any(data != np.floor(data)):
            raise ValueError("histogram: stored bin ids must be integers")
    elif data.dtype.kind not in "iub":
        raise TypeError(f"histogram: unsupported bin dtype {data.dtype}")
    if data.size and data.min() < 0:
        raise ValueError("histogram: stored bin ids must not be negative")
    if B == 65536 and data.size and data.max() > 65535:
        raise ValueError("histogram: with 65536 bins no id is left for a missing value")
    ids = np.minimum(data, B).astype(np.uint8 if B < 256 else np.uint16)
    z = np.asarray(default_bin)
    if z.dtype.kind not in "iu" or z.ndim > 1 or (z.ndim == 1 and z.size != F):
        raise ValueError(f"histogram: default_bin must be an integer or {F} integers")
    z = np.broadcast_to(z.astype(np.int64), (F,))
    zs = np.where((z >= 0) & (z < B), z, -1).astype(np.int32)
    return indptr, indices.astype(np.int32), ids, zs, node, (shape[0], F, B)


def histogram_sparse_counts(indptr, indices, data, zs, node, shape):
    """(counts int64 [cells], stored mask, node per stored entry, row per stored entry): the members of every cell of the
    sparse histogram, default cells included (count(v) minus the stored non-default entries of (v, f)); the mask selects
    the stored entries that enter a slot (valid node, not at the default bin)."""
    nodes, F, B = shape
    N = indptr.size - 1
    v = np.zeros(N, dtype=np.int64) if node is None else node.astype(np.int64)
    okv = (v >= 0) & (v < nodes)
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    f = indices.astype(np.int64)
    b = data.astype(np.int64)
    sel = okv[rows] & ~((b < B) & (b == zs[f]))
    vr = v[rows]
    cell = (vr * F + f) * B + b
    cnt = np.bincount(cell[sel & (b < B)], minlength=nodes * F * B).astype(np.int64).reshape(nodes, F, B)
    stored = np.bincount((vr * F + f)[sel], minlength=nodes * F).astype(np.int64).reshape(nodes, F)
    cv = np.bincount(v[okv], minlength=nodes).astype(np.int64)
    fz = np.flatnonzero(zs >= 0)
    cnt[:, fz, zs[fz]] = cv[:, None] - stored[:, fz]
    return cnt.reshape(-1), sel, vr, rows


def histogram_sparse_words(pk, words, exps, indptr, indices, data, zs, node, shape):
    """(words [cells, W], exponents [cells], counts int64 [cells]) of the sparse histogram over checked arguments:
    pai_histogram_sparse on the GPU, Python integers without one. A cell off the default bin is the product over its
    stored members; a default cell is T_v * invert(S_{v,f})^(16^(E_T - E_S)) at the node's exponent E_T, T_v itself where
    nothing else is stored, and empty (ciphertext 1, EMPTY_EXP) where its count is 0."""
    from . import _runtime
    nodes, F, B = shape
    if _device_words(words):
        from . import device_buffer
        return device_buffer.histogram_sparse_dev(pk, words, exps, indptr, indices, data, zs, node, shape)
    if _runtime.gpu_available():
        return _runtime.context(pk).histogram_sparse(words, exps, indptr, indices, data, F, zs, B, node, nodes)
    W, cells = words.shape[1], nodes * F * B
    cnt, sel, vr, rows = histogram_sparse_counts(indptr, indices, data, zs, node, shape)
    cts, nsq = _ints(words), pk.nsquare
    ex = [int(e) for e in np.asarray(exps).reshape(-1)]

    def fold(members):
        E = max((ex[i] for i in members), default=EMPTY_EXP)
        acc = 1
        for i in members:
            acc = acc * pow(cts[i], 16 ** (E - ex[i]), nsq) % nsq
        return acc, E

    in_cell, in_rest = {}, {}
    for t in np.flatnonzero(sel).tolist():
        v, f, b, i = int(vr[t]), int(indices[t]), int(data[t]), int(rows[t])
        if b < B:
            in_cell.setdefault((v * F + f) * B + b, []).append(i)
        in_rest.setdefault(v * F + f, []).append(i)
    v_of = np.zeros(len(ex), dtype=np.int64) if node is None else node.astype(np.int64)
    totals = [fold(np.flatnonzero(v_of == v).tolist()) for v in range(nodes)]
    acc, oe = [1] * cells, [EMPTY_EXP] * cells
    for s, members in in_cell.items():
        acc[s], oe[s] = fold(members)
    for v in range(nodes):
        for f in np.flatnonzero(zs >= 0).tolist():
            s = (v * F + f) * B + int(zs[f])
            if cnt[s] == 0:
                continue
            (T, ET), rest = totals[v], in_rest.get(v * F + f)
            if rest:
                S, ES = fold(rest)
                try:
                    T = T * pow(pow(S, -1, nsq), 16 ** (ET - ES), nsq) % nsq
                except ValueError as e:
                    raise ZeroDivisionError("invert() no inverse exists") from e
            acc[s], oe[s] = T, ET
    return _runtime.ints_to_words(acc, W).reshape(cells, W), np.array(oe, dtype=np.int32), cnt


def _plain(y, N: int) -> np.ndarray:
    from .cipher_array import _plain_array, _plain_scalar
    if isinstance(y, np.ndarray):
        x = _plain_array(y.reshape(-1))
        if x is None or x.size not in (1, N):
            raise TypeError(f"unsupported plain operand {y.dtype}{y.shape}")
        return x
    dt = _plain_scalar(y)
    if dt is None:
        raise TypeError(f"unsupported plain operand {type(y)}")
    return np.array([y], dtype=dt)


def _item(y, i):
    return y.reshape(-1)[i if y.size > 1 else 0] if isinstance(y, np.ndarray) else y


def _ints(words):
    from . import _runtime
    return _runtime.words_to_ints(words)


def _words(v: int, W: int) -> np.ndarray:
    from . import _runtime
    return _runtime.ints_to_words([v], W)[0]
