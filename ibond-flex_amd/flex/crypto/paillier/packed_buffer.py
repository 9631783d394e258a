"""Packed plaintexts: many signed fixed-point values per Paillier ciphertext (include/flexpai.h, "Packed plaintexts").

A float32 weight uses about 30 of the ~2046 plaintext bits of a 2048-bit key. A PackedLayout cuts the plaintext into
`slots` fields of `slot_bits` bits, each holding one signed fixed-point value t = rint(v * 16^exponent) with
|t| <= 2^(value_bits - 1) - 1; the plaintext is the signed integer M = sum_j t_j 2^(slot_bits j), encrypted like any
other (m = M mod n), so a packed ciphertext is an ordinary ciphertext of the reference: adding two adds every slot,
multiplying by an integer scales every slot. Encrypt, add, obfuscate, decrypt and the wire all shrink by `slots`.

    lay = PackedLayout.for_sum(pub_key, max_abs=4.0, exponent=5, terms=3)   # every party agrees on this
    buf = encryptor.encrypt_packed(weights, lay)                            # ONE pai_encrypt_packed call
    total = add_packed([PackedCiphertextBuffer.from_wire(w) for w in received])   # ONE k-way pai_add call
    send(total.to_wire(be_secure=True))                                     # ONE pai_obfuscate call
    sums = decryptor.decrypt(PackedCiphertextBuffer.from_wire(reply))       # ONE pai_decrypt_packed call

Opt-in, and both peers must be flexpai (like CiphertextBuffer and FLEXPAI_PICKLE_BULK). A slot that overflows into its
neighbour cannot be seen in the plaintext, so every buffer carries `bound`, an exact Python int with |t| <= bound for
every slot: sums add the bounds, products scale them, and a result whose bound would pass 2^(slot_bits - 1) - 1 raises
OverflowError before any GPU call. Only integer scalars are supported (a float scalar would change the exponent of a
whole ciphertext, which the layout fixes).

Results that already exist as ordinary ciphertexts (per-bin sums, integer-weighted sums) are folded into a packed buffer
by a party with the public key only: pack_ciphertexts(src, layout, max_abs), CiphertextBuffer.pack, PaillierArray.pack,
parallel_ops.segment_sum_packed (ONE pai_pack_ciphertexts call: out = prod_j c_j^(2^(slot_bits j))). The caller states
max_abs, since an existing ciphertext cannot show its magnitude. Slots are at most 64 bits wide: integer-valued results
and values of one fixed precision fit, products of two full-precision float encodings (~106-bit mantissas) do not.

Without a GPU the same operations run on Python integers (small arrays only, as in the rest of the package).
"""
from __future__ import annotations

import math
import secrets
from fractions import Fraction
from typing import Optional, Sequence

import numpy as np

from . import _bigint

_MAGIC = b"FPPK1\0"
EL_ENC_RANGE = 5


class PackedLayout(object):
    """(slot_bits, value_bits, exponent, slots) for keys of pub_key's size: slot_bits a multiple of 8 in [16, 64],
    2 <= value_bits <= slot_bits, 1 <= slots <= (key_bits - 2) // slot_bits (the default)."""
    __slots__ = ("slot_bits", "value_bits", "exponent", "slots", "key_bits")

    def __init__(self, pub_key, slot_bits: int, value_bits: int, exponent: int, slots: Optional[int] = None):
        nb = pub_key.n.bit_length()
        slot_bits, value_bits, exponent = int(slot_bits), int(value_bits), int(exponent)
        if slot_bits % 8 or not 16 <= slot_bits <= 64:
            raise ValueError("slot_bits must be a multiple of 8 in [16, 64]")
        if not 2 <= value_bits <= slot_bits:
            raise ValueError("value_bits must be in [2, slot_bits]")
        most = (nb - 2) // slot_bits
        slots = most if slots is None else int(slots)
        if not 1 <= slots <= most:
            raise ValueError(f"slots must be in [1, {most}] for a {nb}-bit key and {slot_bits}-bit slots")
        self.slot_bits, self.value_bits, self.exponent, self.slots, self.key_bits = slot_bits, value_bits, exponent, slots, nb

    @classmethod
    def for_sum(cls, pub_key, max_abs, exponent: int, terms: int = 1) -> "PackedLayout":
        """The layout for sums of `terms` values of magnitude at most max_abs at this exponent: the smallest value_bits
        that hold max_abs * 16^exponent and the smallest slot_bits (a multiple of 8) with ceil(log2 terms) bits above."""
        if terms < 1:
            raise ValueError("terms must be at least 1")
        top = math.ceil(abs(Fraction(max_abs)) * Fraction(16) ** int(exponent))
        value_bits = max(2, int(top).bit_length() + 1)
        head = (int(terms) - 1).bit_length()
        slot_bits = max(16, -(-(value_bits + head) // 8) * 8)
        if slot_bits > 64:
            raise ValueError("max_abs * 16^exponent * terms does not fit a 64-bit slot")
        return cls(pub_key, slot_bits, value_bits, exponent)

    @property
    def value_max(self) -> int:
        return (1 << (self.value_bits - 1)) - 1

    @property
    def slot_max(self) -> int:
        return (1 << (self.slot_bits - 1)) - 1

    def as_tuple(self):
        return self.slot_bits, self.value_bits, self.exponent, self.slots

    def __eq__(self, other):
        return isinstance(other, PackedLayout) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def __repr__(self):
        return "PackedLayout(slot_bits=%d, value_bits=%d, exponent=%d, slots=%d)" % self.as_tuple()


# ---------------------------------------------------------------- the contract on Python integers (no GPU)
def pack_int(ts: Sequence[int], slot_bits: int) -> int:
    """M = sum_j t_j 2^(slot_bits j): signed, slot 0 least significant."""
    M = 0
    for j, t in enumerate(ts):
        M += int(t) << (slot_bits * j)
    return M


def unpack_int(m: int, n: int, slot_bits: int, slots: int):
    """The signed digits of the raw plaintext m in [0, n), or None where decoding overflows."""
    max_int = n // 3 - 1
    if m <= max_int:
        M = m
    elif m >= n - max_int:
        M = m - n
    else:
        return None
    B, out = 1 << slot_bits, []
    for _ in range(slots):
        t = ((M + B // 2) % B) - B // 2
        out.append(t)
        M = (M - t) // B
    return out if M == 0 else None


def encode_values(x: np.ndarray, layout: PackedLayout):
    """(t as Python ints, statuses) of a float32 / float64 / int64 array at the layout's exponent, as the device
    encodes them; a value out of range is 0 with status EL_ENC_RANGE."""
    e, lim = layout.exponent, layout.value_max
    ts, st = [], []
    for v in x.reshape(-1).tolist():
        if isinstance(v, float):
            if math.isnan(v) or math.isinf(v):
                t = None
            else:
                t = 0 if abs(v) < 1e-200 else round(math.ldexp(v, 4 * e))
        else:
            t = v << (4 * e) if e >= 0 else round(math.ldexp(float(v), 4 * e))
        bad = t is None or abs(t) > lim
        ts.append(0 if bad else t)
        st.append(EL_ENC_RANGE if bad else 0)
    return ts, st


def _ints(words):
    from . import _runtime
    return _runtime.words_to_ints(words)


def _to_words(vals, W):
    from . import _runtime
    return _runtime.ints_to_words(vals, W)


def _gpu() -> bool:
    from . import _runtime
    return _runtime.gpu_available()


def _resident(words) -> bool:
    """True when the words are a device holder (device_buffer.DeviceWords), not a numpy array."""
    if isinstance(words, np.ndarray):
        return False
    from .device_buffer import DeviceWords
    return isinstance(words, DeviceWords)


def host_raw_decrypt(c: int, priv_key) -> int:
    """decryptor.py:33-63 on Python integers: the raw plaintext in [0, n)."""
    p, q = priv_key.p, priv_key.q
    mp = (_bigint.powmod(c, p - 1, priv_key.psquare) - 1) // p * priv_key.hp % p
    mq = (_bigint.powmod(c, q - 1, priv_key.qsquare) - 1) // q * priv_key.hq % q
    return _bigint.crt(mp, mq, p, q, priv_key.q_inverse, priv_key.public_key.n)


class PackedCiphertextBuffer(object):
    """C = ceil(count / slots) packed ciphertexts: words [C, W], the layout, the number of values and their shape, one
    obfuscation flag for the buffer, and the exact slot bound. to_device() gives the same buffer with its words resident
    on the GPU (device_buffer.DeviceWords in the place of the numpy words): the operators then run the *_dev entry
    points and return resident buffers; layout and bound bookkeeping are the same, checked before any GPU call."""
    __slots__ = ("public_key", "words", "layout", "count", "shape", "obfuscated", "bound")

    def __init__(self, public_key, words: np.ndarray, layout: PackedLayout, count: int, shape=None,
                 obfuscated: bool = False, bound: Optional[int] = None):
        nb = public_key.n.bit_length()
        W = (2 * nb + 31) // 32
        if not isinstance(layout, PackedLayout) or layout.key_bits != nb:
            raise ValueError("layout does not belong to a key of this size")
        if not _resident(words):
            words = np.ascontiguousarray(words, dtype=np.uint32)
        count = int(count)
        C = -(-count // layout.slots)
        if tuple(words.shape) != (C, W):
            raise ValueError(f"ciphertext words {words.shape} do not match ({C}, {W}) for {count} values")
        self.public_key, self.words, self.layout, self.count = public_key, words, layout, count
        self.shape = tuple(int(v) for v in shape) if shape is not None else (count,)
        if int(np.prod(self.shape, dtype=np.int64)) != count:
            raise ValueError("shape does not match the number of values")
        self.obfuscated = bool(obfuscated)
        self.bound = layout.value_max if bound is None else int(bound)
        if not 0 <= self.bound <= layout.slot_max:
            raise OverflowError(f"slot bound {self.bound} exceeds 2^(slot_bits - 1) - 1")

    def __repr__(self):
        where = ", resident" if self.resident else ""
        return f"PackedCiphertextBuffer(shape={self.shape}, {self.layout!r}, bound={self.bound}{where})"

    @property
    def resident(self) -> bool:
        return _resident(self.words)

    def to_device(self) -> "PackedCiphertextBuffer":
        """The same buffer with its words on the GPU (one upload; RuntimeError without a GPU)."""
        if self.resident:
            return self
        from . import _runtime
        from .cipher_buffer import need_gpu
        from .device_buffer import DeviceWords
        need_gpu()
        return self._like(DeviceWords.from_host(self.words, _runtime.context(self.public_key).device), self.bound,
                          self.obfuscated)

    def to_host(self) -> "PackedCiphertextBuffer":
        """The same buffer with numpy words (one download)."""
        return self._like(self.words.to_host(), self.bound, self.obfuscated) if self.resident else self

    @property
    def size(self) -> int:
        return self.count

    def _like(self, words, bound, obfuscated=False):
        return PackedCiphertextBuffer(self.public_key, words, self.layout, self.count, self.shape, obfuscated, bound)

    def _exps(self):
        return np.full(self.words.shape[0], self.layout.exponent, dtype=np.int32)

    def _check_peer(self, other):
        if not isinstance(other, PackedCiphertextBuffer):
            raise TypeError(f"unsupported operand {type(other)} for a packed buffer")
        if other.public_key != self.public_key:
            raise ValueError("add two numbers have different public key!")
        if other.layout != self.layout:
            raise ValueError(f"layouts differ: {self.layout!r} and {other.layout!r}")
        if other.shape != self.shape:
            raise ValueError(f"shapes {self.shape} and {other.shape} differ")

    def _check_bound(self, bound: int):
        if bound > self.layout.slot_max:
            raise OverflowError(f"slot bound {bound} would exceed 2^{self.layout.slot_bits - 1} - 1: a slot could "
                                "overflow into its neighbour")

    # ---------------------------------------------------------------- operators
    def __add__(self, other):
        return add_packed([self, other])

    def __sub__(self, other):
        self._check_peer(other)
        self._check_bound(self.bound + other.bound)
        return add_packed([self, other * -1])

    def __mul__(self, s):
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)):
            raise TypeError("a packed buffer multiplies by integers only (a float would change the exponent)")
        s = int(s)
        if abs(s) >= 1 << 63:
            raise OverflowError("scalar must be below 2^63 in magnitude")
        bound = self.bound * abs(s)
        self._check_bound(bound)
        if self.resident:
            from .device_buffer import mul_dev
            out, _, _ = mul_dev(self.public_key, self.words, self._exps(), np.array([s], dtype=np.int64))
        elif _gpu():
            from . import _runtime
            out, _, _ = _runtime.context(self.public_key).mul(self.words, self._exps(), np.array([s], dtype=np.int64))
        else:
            nsq = self.public_key.nsquare
            out = _to_words([_bigint.scalar_pow(c, abs(s), nsq, s < 0) if s else 1 for c in _ints(self.words)],
                            self.words.shape[1])
        return self._like(out, bound)

    __rmul__ = __mul__

    def histogram(self, bins, n_bins: int, node=None, n_nodes: int = 1, default_bin=0):
        """Histogram of samples encrypted as packed ciphertexts, ONE ciphertext per sample (count == samples * slots:
        g and h of a sample in two slots): (PackedCiphertextBuffer of shape (n_nodes, F, n_bins, slots) with this layout,
        int64 counts of shape (n_nodes, F, n_bins)) from one pai_histogram call, every slot summed per cell at once. The
        bound is this buffer's bound * counts.max(); the counts are taken on the host first, so that OverflowError is
        raised before any GPU call if it passes the slot. Empty cells decode as 0 in every slot.
        On a resident buffer, dense bins (uint8 / uint16, C-contiguous [N, F]) and node (int32 [N]) may be
        device_buffer.DeviceArrays: nothing is uploaded for them. Their cells cannot be counted on the host, so the
        buffer's bound times ALL its samples must fit the slot (OverflowError otherwise).
        Sparse bins (anything that offers .tocsr()) take one pai_histogram_sparse call with default_bin as in
        CiphertextBuffer.histogram; a packed buffer's exponents are uniform, so the bits are the dense call's."""
        from .cipher_buffer import (histogram_args, histogram_cells, histogram_sparse_args, histogram_sparse_counts,
                                    histogram_sparse_words, histogram_words, sparse_csr)
        k, N = self.layout.slots, self.words.shape[0]
        if self.count != N * k:
            raise ValueError(f"histogram: {self.count} values do not fill {N} ciphertexts of {k} slots (one ciphertext "
                             "per sample; a buffer after repack() no longer has one)")
        # After repack() a ciphertext holds several whole rows of the last axis (k = slots of a row * g), and count can be
        # a multiple of k again (300 samples of 2 slots at g = 10: 30 ciphertexts of 20): each would mix g samples.
        if len(self.shape) >= 2 and self.shape[-1] != k and self.shape[-1] > 0 and k % self.shape[-1] == 0:
            raise ValueError(f"histogram: a ciphertext of {k} slots spans {k // self.shape[-1]} rows of shape {self.shape}: "
                             "one ciphertext per sample is needed (repack() goes after histogram)")
        # A resident buffer whose bound times ALL its samples fits the slot cannot overflow whatever the cells are: that
        # check replaces the host-side count (22 ms for 262 144 x 16 bin ids, more than the kernels), and the counts the
        # device returns give the same exact bound afterwards. Every other case counts on the host first, as before.
        safe = self.resident and self.bound * N <= self.layout.slot_max
        from .device_buffer import DeviceArray, histogram_resident_args
        on_device = isinstance(bins, DeviceArray) or isinstance(node, DeviceArray)
        csr = None if isinstance(bins, DeviceArray) else sparse_csr(bins)
        if on_device and csr is not None:
            raise TypeError("histogram: sparse bins take host node ids")
        if on_device and not self.resident:
            raise TypeError("histogram: DeviceArray operands need a resident buffer (to_device())")
        if on_device and not safe:
            # the exact bound needs the counts before the call, and the operands are not on the host
            raise OverflowError(f"histogram: bound {self.bound} x {N} samples passes the slot, and the cells of DeviceArray "
                                "operands cannot be counted on the host first: pass host bins and node ids")
        if csr is not None:
            # (a default cell is a true subset sum, T_v minus the stored rest, so counts.max() bounds it like any cell)
            *args, shape = histogram_sparse_args(N, csr, n_bins, node, n_nodes, default_bin)
            cells = shape[0] * shape[1] * shape[2]
            if not safe:
                cnt = histogram_sparse_counts(*args, shape)[0]
                self._check_bound(self.bound * (int(cnt.max()) if cnt.size else 0))
            out, _, dev_cnt = histogram_sparse_words(self.public_key, self.words, self._exps(), *args, shape)
        else:
            b, nd, shape = (histogram_resident_args if on_device else histogram_args)(N, bins, n_bins, node, n_nodes)
            cells = shape[0] * shape[1] * shape[2]
            if not safe:
                cell = histogram_cells(b, shape[2], nd, shape[0])
                cnt = np.bincount(cell[cell >= 0], minlength=cells).astype(np.int64)
                self._check_bound(self.bound * (int(cnt.max()) if cnt.size else 0))
            out, _, dev_cnt = histogram_words(self.public_key, self.words, self._exps(), b, shape[2], nd, shape[0])
        if safe:
            cnt = dev_cnt
        bound = self.bound * (int(cnt.max()) if cnt.size else 0)
        return (PackedCiphertextBuffer(self.public_key, out, self.layout, cells * k, shape + (k,), False, bound),
                cnt.reshape(shape))

    def cumsum(self, axis: int, reverse: bool = False) -> "PackedCiphertextBuffer":
        """Running sums along a leading axis (reverse: from the end), every slot at once, in ONE pai_cumsum call; for
        buffers whose last axis is exactly the slots of one ciphertext per index of the leading axes, which is what
        histogram returns (ValueError for any other shape, and for the slot axis). The bound is this buffer's bound * the
        length of the axis: the layout must be sized for the cumulated sums; OverflowError, before any GPU call, if it
        passes the slot. Not obfuscated."""
        from .cipher_buffer import axis_split, cumsum_words
        k, C = self.layout.slots, self.words.shape[0]
        if len(self.shape) < 2 or self.shape[-1] != k or self.count != C * k:
            raise ValueError(f"cumsum: shape {self.shape} is not (..., {k}) with one ciphertext per index of the leading axes "
                             "(repack() goes after cumsum)")
        lead = self.shape[:-1]
        outer, L, inner = axis_split(lead, axis)
        bound = self.bound * L
        self._check_bound(bound)
        out, _ = cumsum_words(self.public_key, self.words, self._exps(), outer, L, inner, bool(reverse))
        return self._like(out, bound)

    def repack(self, slots: Optional[int] = None) -> "PackedCiphertextBuffer":
        """The same values in fewer, fuller ciphertexts (SecureBoost+'s cipher compression): `slots` per ciphertext, a
        multiple of layout.slots (default: the largest that fits (key_bits - 2) // slot_bits), from ONE pai_repack call,
        out_c = prod_j c_(c g + j)^(2^(layout.slots slot_bits j)) with g = slots // layout.slots; needs the public key
        only. Value i stays value i: count, shape and bound are kept, the layout becomes (slot_bits, value_bits, exponent,
        slots), and decrypt gives exactly what it gives for this buffer. The result is NOT re-randomised
        (obfuscated=False; to_wire(be_secure=True) does that), so repack goes after the last histogram / cumsum / take --
        which address whole ciphertexts along axes of `shape` and refuse a repacked buffer -- and before the
        re-randomisation. slots == layout.slots returns self; a resident buffer stays resident."""
        lay = self.layout
        s, most = lay.slots, (lay.key_bits - 2) // lay.slot_bits
        slots = most // s * s if slots is None else int(slots)
        if slots < s or slots % s:
            raise ValueError(f"repack: slots must be a multiple of the layout's {s} slots, not {slots}")
        if slots > most:
            raise ValueError(f"repack: {slots} slots of {lay.slot_bits} bits do not fit a {lay.key_bits}-bit key (at most {most})")
        if slots == s:
            return self
        g = slots // s
        if self.resident:
            from .device_buffer import repack_dev
            out = repack_dev(self.public_key, self.words, lay, g)
        elif self.words.shape[0] == 0:
            out = self.words
        elif _gpu():
            from . import _runtime
            out = _runtime.context(self.public_key).repack(self.words, lay, g)
        else:
            out = _to_words(host_repack(_ints(self.words), lay, g, self.public_key), self.words.shape[1])
        wide = PackedLayout(self.public_key, lay.slot_bits, lay.value_bits, lay.exponent, slots)
        return PackedCiphertextBuffer(self.public_key, out, wide, self.count, self.shape, False, self.bound)

    def apply_obfuscation(self) -> "PackedCiphertextBuffer":
        """Re-randomise every ciphertext in ONE pai_obfuscate call, unless the flag is already set. Returns self."""
        if self.obfuscated or self.words.shape[0] == 0:
            self.obfuscated = True
            return self
        if self.resident:
            from .device_buffer import obfuscate_dev
            self.words = obfuscate_dev(self.public_key, self.words)
        elif _gpu():
            from .obfuscator import apply_obfuscation_array
            self.words = apply_obfuscation_array(self.words, self.public_key)
        else:
            n, nsq = self.public_key.n, self.public_key.nsquare
            self.words = _to_words([c * _bigint.powmod(secrets.randbelow(n - 1) + 1, n, nsq) % nsq
                                    for c in _ints(self.words)], self.words.shape[1])
        self.obfuscated = True
        return self

    # ---------------------------------------------------------------- wire
    def to_wire(self, be_secure: bool = False) -> bytes:
        """magic | u32 n bytes | n | u32 W | i32 slot_bits, value_bits, exponent, slots | u64 count | u32 ndim |
        i64 shape[ndim] | u32 bound bytes | bound | u8 flags (bit 0: obfuscated) | u32 words[C][W], little-endian.
        be_secure=True: apply_obfuscation() first."""
        if be_secure:
            self.apply_obfuscation()
        n = self.public_key.n
        nbytes = (n.bit_length() + 7) // 8
        bb = max(1, (self.bound.bit_length() + 7) // 8)
        return b"".join([_MAGIC, np.uint32(nbytes).tobytes(), n.to_bytes(nbytes, "little"),
                         np.uint32(self.words.shape[1]).tobytes(),
                         np.asarray(self.layout.as_tuple(), dtype="<i4").tobytes(), np.uint64(self.count).tobytes(),
                         np.uint32(len(self.shape)).tobytes(), np.asarray(self.shape, dtype="<i8").tobytes(),
                         np.uint32(bb).tobytes(), self.bound.to_bytes(bb, "little"),
                         bytes([1 if self.obfuscated else 0]),
                         np.ascontiguousarray(self.words.to_host() if self.resident else self.words, dtype="<u4").tobytes()])

    def take(self, indices, axis: int = 0) -> "PackedCiphertextBuffer":
        """np.take along a leading axis, for buffers whose last axis is exactly the slots of one ciphertext per index of
        the leading axes (what histogram returns); the slot axis cannot be indexed. One pai_take_dev on a resident
        buffer."""
        from .cipher_buffer import axis_split
        k, C = self.layout.slots, self.words.shape[0]
        if len(self.shape) < 2 or self.shape[-1] != k or self.count != C * k:
            raise ValueError(f"take: shape {self.shape} is not (..., {k}) with one ciphertext per index of the leading axes "
                             "(repack() goes after take)")
        lead = self.shape[:-1]
        axis_split(lead, axis)                                                  # (the axis rules; the slot axis is out)
        idx = np.take(np.arange(C, dtype=np.int64).reshape(lead), indices, axis=axis)
        if self.resident:
            from .device_buffer import take_dev
            words, _ = take_dev(self.public_key, self.words, self._exps(), idx.reshape(-1))
        else:
            words = self.words[idx.reshape(-1)]
        return PackedCiphertextBuffer(self.public_key, words, self.layout, idx.size * k, idx.shape + (k,), self.obfuscated,
                                      self.bound)

    @classmethod
    def from_wire(cls, buf, public_key=None, device: bool = False) -> "PackedCiphertextBuffer":
        """Inverse of to_wire. `public_key` (optional) must match the key in the buffer. ValueError for anything
        malformed: a wrong length or W, an invalid layout, a count above C * slots, a bound above the slot, a word row
        >= n^2. device=True: a resident buffer; the words are uploaded once and range-checked on the GPU."""
        from .cipher_array import _rows_below
        from .keypair import PaillierPublicKey
        mv = memoryview(buf).cast("B")
        bad = ValueError("corrupted packed ciphertext buffer")
        if len(mv) < len(_MAGIC) + 4 or bytes(mv[:len(_MAGIC)]) != _MAGIC:
            raise ValueError("not a flexpai packed ciphertext buffer")
        o = len(_MAGIC)

        def take(dtype, cnt=1):
            nonlocal o
            size = np.dtype(dtype).itemsize * cnt
            if cnt < 0 or len(mv) < o + size:
                raise bad
            out = np.frombuffer(mv, dtype, cnt, o)
            o += size
            return out

        nbytes = int(take("<u4")[0])
        if nbytes == 0 or nbytes > 1024:
            raise bad
        n = int.from_bytes(take(np.uint8, nbytes).tobytes(), "little")
        W = int(take("<u4")[0])
        if n < 3 or W != (2 * n.bit_length() + 31) // 32:
            raise bad
        sb, vb, e, k = (int(v) for v in take("<i4", 4))
        count = int(take("<u8")[0])
        ndim = int(take("<u4")[0])
        if ndim > 32:
            raise bad
        shape = tuple(int(v) for v in take("<i8", ndim))
        bb = int(take("<u4")[0])
        if bb == 0 or bb > 16:
            raise bad
        bound = int.from_bytes(take(np.uint8, bb).tobytes(), "little")
        flags = int(take(np.uint8)[0])
        if public_key is None:
            public_key = PaillierPublicKey(n)
        elif public_key.n != n:
            raise ValueError("packed ciphertext buffer was encrypted under a different public key")
        try:
            layout = PackedLayout(public_key, sb, vb, e, k)
        except ValueError:
            raise bad from None
        if any(v < 0 for v in shape) or (int(np.prod(shape, dtype=object)) if shape else 1) != count or flags > 1:
            raise bad
        if (len(mv) - o) % (4 * W):
            raise ValueError("corrupted packed ciphertext buffer (length mismatch)")
        C = (len(mv) - o) // (4 * W)
        if count > C * k or C != -(-count // k):
            raise ValueError("corrupted packed ciphertext buffer (count does not match the ciphertexts)")
        if bound > layout.slot_max:
            raise ValueError("corrupted packed ciphertext buffer (bound above the slot)")
        if device:
            from . import _runtime
            from .cipher_buffer import need_gpu
            from .device_buffer import upload_checked
            need_gpu()
            words = upload_checked(public_key, take("<u4", C * W).reshape(C, W), _runtime.context(public_key).device,
                                   "corrupted packed ciphertext buffer (ciphertext >= n^2)")
            return cls(public_key, words, layout, count, shape, bool(flags & 1), bound)
        words = take("<u4", C * W).reshape(C, W).copy()
        if C and not _rows_below(words, public_key.nsquare):
            raise ValueError("corrupted packed ciphertext buffer (ciphertext >= n^2)")
        return cls(public_key, words, layout, count, shape, bool(flags & 1), bound)


def add_packed(bufs: Sequence[PackedCiphertextBuffer]) -> PackedCiphertextBuffer:
    """Slot-wise sum of k packed buffers of one key, layout and shape in ONE k-way add (equal exponents: no alignment).
    The bound of the sum is the sum of the bounds; OverflowError, before any GPU call, if it passes the slot."""
    bufs = list(bufs)
    if not bufs:
        raise ValueError("add_packed needs at least one buffer")
    a = bufs[0]
    if not isinstance(a, PackedCiphertextBuffer):
        raise TypeError(f"unsupported operand {type(a)} for a packed buffer")
    for b in bufs[1:]:
        a._check_peer(b)
    bound = sum(b.bound for b in bufs)
    a._check_bound(bound)
    if len(bufs) == 1:
        return a
    if any(b.resident for b in bufs):          # one resident operand keeps the sum on the device
        from .device_buffer import add_dev
        out, _ = add_dev(a.public_key, [b.to_device().words for b in bufs], [a._exps()] * len(bufs))
    elif _gpu():
        from . import _runtime
        out, _ = _runtime.context(a.public_key).add([b.words for b in bufs], [a._exps()] * len(bufs))
    else:
        nsq = a.public_key.nsquare
        rows = [_ints(b.words) for b in bufs]
        out = _to_words([math.prod(col) % nsq for col in zip(*rows)], a.words.shape[1])
    return a._like(out, bound)


def host_encrypt_packed(x: np.ndarray, layout: PackedLayout, pub_key):
    """encrypt_packed on Python integers: (words, statuses)."""
    ts, st = encode_values(x, layout)
    n, nsq, k = pub_key.n, pub_key.nsquare, layout.slots
    cts = []
    for c in range(-(-len(ts) // k)):
        m = pack_int(ts[c * k:(c + 1) * k], layout.slot_bits) % n
        cts.append((1 + n * m) % nsq * _bigint.powmod(secrets.randbelow(n - 1) + 1, n, nsq) % nsq)
    return _to_words(cts, (2 * n.bit_length() + 31) // 32), np.array(st, dtype=np.int32)


_EMPTY_EXP = -(1 << 31)     # the exponent of pai_segment_add's empty segment (ciphertext 1)


def host_pack_ciphertexts(cts: Sequence[int], exps: Sequence[int], layout: PackedLayout, pub_key):
    """pai_pack_ciphertexts on Python integers: (packed ciphertext ints, statuses). Value i contributes
    c_i^(16^D * 2^(slot_bits j)) to output i // slots, j = i % slots, D = layout.exponent - exps[i] with
    0 <= 4 D < slot_bits; an empty segment contributes 1; any other exponent is EL_ENC_RANGE and contributes 1."""
    nsq, k, sb, E = pub_key.nsquare, layout.slots, layout.slot_bits, layout.exponent
    out, st = [1] * -(-len(cts) // k), []
    for i, (c, e) in enumerate(zip(cts, exps)):
        e = int(e)
        d = E - e
        if e == _EMPTY_EXP:
            st.append(0)
        elif d < 0 or 4 * d >= sb:
            st.append(EL_ENC_RANGE)
        else:
            st.append(0)
            out[i // k] = out[i // k] * _bigint.powmod(int(c), 1 << (4 * d + sb * (i % k)), nsq) % nsq
    return out, np.array(st, dtype=np.int32)


def host_repack(cts: Sequence[int], layout: PackedLayout, group: int, pub_key):
    """pai_repack on Python integers: packed ciphertext c_i under `layout` contributes c_i^(2^(slots slot_bits j)) to
    output i // group, j = i % group."""
    nsq, g, stride = pub_key.nsquare, int(group), layout.slots * layout.slot_bits
    if g < 1 or layout.slots * g > (layout.key_bits - 2) // layout.slot_bits:
        raise ValueError("repack: slots * group must be in [slots, (key_bits - 2) // slot_bits]")
    out = [1] * -(-len(cts) // g)
    for i, c in enumerate(cts):
        out[i // g] = out[i // g] * _bigint.powmod(int(c), 1 << (stride * (i % g)), nsq) % nsq
    return out


def _slot_bound(layout: PackedLayout, max_abs, terms: int = 1) -> int:
    """terms * ceil(max_abs * 16^exponent), or OverflowError where that passes the slot."""
    if not isinstance(layout, PackedLayout):
        raise ValueError("layout does not belong to a key of this size")
    bound = int(terms) * math.ceil(abs(Fraction(max_abs)) * Fraction(16) ** layout.exponent)
    if bound > layout.slot_max:
        raise OverflowError(f"slot bound {bound} would exceed 2^{layout.slot_bits - 1} - 1: a slot could overflow "
                            "into its neighbour")
    return bound


def _fold(pub_key, words, exps, layout: PackedLayout, bound: int, shape) -> "PackedCiphertextBuffer":
    """One pai_pack_ciphertexts call over words [N, W] / exps [N] (Python integers without a GPU); resident words
    (device_buffer.DeviceWords) fold on the device into a resident buffer."""
    if not isinstance(layout, PackedLayout) or layout.key_bits != pub_key.n.bit_length():
        raise ValueError("layout does not belong to a key of this size")
    W = (2 * pub_key.n.bit_length() + 31) // 32
    if _resident(words):
        from .device_buffer import pack_dev
        out, st = pack_dev(pub_key, words, exps, layout)
    elif exps.size == 0:
        out, st = np.zeros((0, W), dtype=np.uint32), np.zeros(0, dtype=np.int32)
    elif _gpu():
        from . import _runtime
        out, st = _runtime.context(pub_key).pack_ciphertexts(words, exps, layout)
    else:
        ints, st = host_pack_ciphertexts(_ints(words), exps.tolist(), layout, pub_key)
        out = _to_words(ints, W)
    bad = np.flatnonzero(st)
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"pack_ciphertexts: value at index {i} has exponent {int(exps[i])}, outside the layout's range "
                         f"(0 <= 4 * ({layout.exponent} - exponent) < {layout.slot_bits})")
    return PackedCiphertextBuffer(pub_key, out, layout, int(exps.size), shape, obfuscated=False, bound=bound)


def pack_ciphertexts(src, layout: PackedLayout, max_abs) -> "PackedCiphertextBuffer":
    """Fold EXISTING ordinary ciphertexts (a CiphertextBuffer, a PaillierArray or an object array of
    PaillierEncryptedNumber) into a PackedCiphertextBuffer under `layout`, layout.slots per ciphertext, in ONE
    pai_pack_ciphertexts call; needs the public key only. The values must be integers at the layout's exponent, and the
    caller vouches for |value| <= max_abs, which an existing ciphertext cannot show: the buffer's bound is
    ceil(max_abs * 16^exponent), OverflowError before any GPU call if that passes the slot. Every exponent must satisfy
    0 <= 4 (layout.exponent - exponent) < slot_bits (ValueError names the first index that does not). The result is not
    re-randomised (obfuscated=False): to_wire(be_secure=True) does that."""
    from .cipher_buffer import CiphertextBuffer
    from .device_buffer import DeviceCiphertextBuffer
    if isinstance(src, (CiphertextBuffer, DeviceCiphertextBuffer)):
        pk, words, exps, shape = src.public_key, src.words, src.exps, src.shape
    elif isinstance(src, np.ndarray) and src.dtype == object:
        from .cipher_array import _encrypted_operand, pack
        A, pk = _encrypted_operand(src)
        if A is None:
            raise TypeError("pack_ciphertexts needs a non-empty array of PaillierEncryptedNumber with one public key")
        words, exps, _ = pack(src, pk)
        shape = A.shape
    else:
        raise TypeError(f"unsupported operand {type(src)} for pack_ciphertexts")
    if not isinstance(layout, PackedLayout) or layout.key_bits != pk.n.bit_length():
        raise ValueError("layout does not belong to a key of this size")
    bound = _slot_bound(layout, max_abs)
    return _fold(pk, words, np.ascontiguousarray(exps, dtype=np.int32).reshape(-1), layout, bound, shape)


def host_decrypt_packed(buf: PackedCiphertextBuffer, priv_key):
    """decrypt_packed on Python integers: the slot integers, or OverflowError."""
    lay, n = buf.layout, buf.public_key.n
    ts = []
    for c in _ints(buf.words):
        row = unpack_int(host_raw_decrypt(c, priv_key), n, lay.slot_bits, lay.slots)
        if row is None:
            raise OverflowError('Overflow detected in decode number')
        ts += row
    return ts[:buf.count]
