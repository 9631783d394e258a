"""parallel_ops — same API as flex/crypto/paillier/parallel_ops.py:23-129.

enc + enc arrays run as one batched GPU add (cipher_array.add_encrypted) and enc * plain as one
batched GPU multiply (cipher_array.mul_plain) instead of one ProcessPoolExecutor task per element;
enc + plain as one batched GPU encode + add (cipher_array.add_plain)."""
from typing import Union

import numpy as np

from .cipher_array import PaillierArray, add_encrypted, add_plain, mul_plain


def mul(x: np.ndarray, y: Union[np.ndarray, float, int]) -> np.ndarray:
    return calculate(x, y, 'mul')


def add(x: np.ndarray, y: Union[np.ndarray, float, int]) -> np.ndarray:
    return calculate(x, y, 'add')


def _add(x, y):
    return x + y


def _mul(x, y):
    return x * y


def calculate(x: np.ndarray, y: Union[np.ndarray, float, int], method: str) -> np.ndarray:
    if not isinstance(x, np.ndarray):
        # the reference raises ValueError(msg=...), which Python turns into a TypeError
        raise TypeError(f"{type(x)} * {type(y)} not supported")
    if method == 'add':
        func = _add
    elif method == 'mul':
        func = _mul
    else:
        raise NotImplementedError(method)
    if isinstance(y, np.ndarray) and x.shape != y.shape:
        raise TypeError(f"{x.shape} != {y.shape}")
    if method == 'add' and isinstance(y, np.ndarray) and y.dtype == object:
        res = add_encrypted(x, y)
        if res is not NotImplemented:
            return res.reshape(x.shape)
    if method == 'add' and (isinstance(y, (int, float)) or (isinstance(y, np.ndarray) and y.dtype != object)):
        res = add_plain(x, y)                    # one encode launch + one 2-way k_add
        if res is not NotImplemented:
            return res.reshape(x.shape)
    if method == 'mul' and (isinstance(y, (int, float)) or (isinstance(y, np.ndarray) and y.dtype != object)):
        res = mul_plain(x, y)                    # one GPU launch instead of a task per element
        if res is not NotImplemented:
            return res.reshape(x.shape)
    xf = np.asarray(x).reshape(-1)
    if isinstance(y, (int, float)):
        out = [func(a, y) for a in xf]
    else:
        yf = np.asarray(y).reshape(-1)
        out = [func(a, b) for a, b in zip(xf, yf)]
    return np.array(out).reshape(x.shape)


def segment_sum(x: np.ndarray, index_lists) -> list:
    """``[sum(x[i]) for i in index_lists]`` (the per-bin sums of hetero_bin.py:28-36) as ONE segmented
    k-way add on the GPU (pai_segment_add) followed by ``0 + S`` (one batched add_plain, which raises a
    segment whose exponent is negative to 0 exactly like Python's sum starting from int 0). Empty
    segments give the int 0, as ``sum([])`` does."""
    from . import _runtime
    from .cipher_array import _encrypted_operand, materialize, pack
    lists = [np.asarray(i).reshape(-1) for i in index_lists]
    flat = np.asarray(x).reshape(-1)
    A, pk = _encrypted_operand(flat)
    if A is None:
        return [sum(flat[i]) for i in lists]
    sizes = np.array([len(i) for i in lists], dtype=np.int64)
    idx = np.concatenate(lists).astype(np.int64) if sizes.sum() else np.zeros(0, dtype=np.int64)
    idx = np.where(idx < 0, idx + flat.size, idx)          # numpy negative indices, like x[i]
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    words, exps, _ = pack(x, pk)
    ctx = _runtime.context(pk)
    out, oe = ctx.segment_add(words, exps, idx, seg_off)
    nz = np.flatnonzero(sizes)
    res = [0] * len(lists)
    if nz.size:
        sums = materialize(pk, out[nz], oe[nz], (nz.size,), obfuscated=False)
        total = add_plain(sums, 0)                          # Python's sum starts from the int 0
        for k, s in zip(nz.tolist(), np.asarray(total).reshape(-1)):
            res[k] = s
    return res


def cumsum(x: np.ndarray, axis: int = -1, reverse: bool = False) -> PaillierArray:
    """``np.cumsum(x, axis)`` of an object array of PaillierEncryptedNumber under one key (reverse: the running sums from
    the end of the axis) as ONE pai_cumsum call: each element is the reference's __add__ chain over its prefix, not
    obfuscated. Without a GPU the same runs on Python integers."""
    from .cipher_array import _encrypted_operand, materialize, pack
    from .cipher_buffer import axis_split, cumsum_words
    if _on_device(x):
        return x.cumsum(axis, reverse)                      # a device buffer in, a device buffer out
    if not isinstance(x, np.ndarray):
        raise TypeError(f"cumsum of {type(x)} not supported")
    A, pk = _encrypted_operand(x)
    if A is None or A.ndim == 0:
        raise TypeError("cumsum needs a non-empty array of PaillierEncryptedNumber with one public key")
    outer, L, inner = axis_split(A.shape, axis)
    words, exps, _ = pack(x, pk)
    out, oe = cumsum_words(pk, words, exps, outer, L, inner, bool(reverse))
    return materialize(pk, out, oe, A.shape, obfuscated=False)


def segment_dot(x: np.ndarray, index_lists, weight_lists) -> list:
    """``[sum(x[i] * w for i, w in zip(idx, ws)) for idx, ws in zip(index_lists, weight_lists)]`` (weighted per-bin sums,
    sparse gradient columns) as ONE segmented weighted sum on the GPU (pai_segment_dot), shaped like segment_sum: the
    ``0 + S`` of Python's sum follows as one batched add_plain, and an empty segment gives the int 0. Without a GPU the
    same runs on Python integers."""
    from .cipher_array import _encrypted_operand, materialize, pack
    from .cipher_buffer import segment_dot_args, segment_dot_words
    lists = [np.asarray(i).reshape(-1) for i in index_lists]
    wlists = [np.asarray(w).reshape(-1) for w in weight_lists]
    if len(lists) != len(wlists) or any(i.size != w.size for i, w in zip(lists, wlists)):
        raise ValueError("segment_dot: index_lists and weight_lists differ in shape")
    flat = np.asarray(x).reshape(-1)
    A, pk = _encrypted_operand(flat)
    if A is None:
        return [sum(flat[i] * w for i, w in zip(idx.tolist(), ws)) for idx, ws in zip(lists, wlists)]
    sizes = np.array([len(i) for i in lists], dtype=np.int64)
    idx = np.concatenate(lists).astype(np.int64) if sizes.sum() else np.zeros(0, dtype=np.int64)
    idx = np.where(idx < 0, idx + flat.size, idx)          # numpy negative indices, like x[i]
    wts = np.concatenate(wlists) if sizes.sum() else np.zeros(0, dtype=np.float64)
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    words, exps, _ = pack(x, pk)
    out, oe = segment_dot_words(pk, words, exps, *segment_dot_args(exps.size, idx, seg_off, wts))
    nz = np.flatnonzero(sizes)
    res = [0] * len(lists)
    if nz.size:
        sums = materialize(pk, out[nz], oe[nz], (nz.size,), obfuscated=False)
        total = add_plain(sums, 0)                          # Python's sum starts from the int 0
        if total is NotImplemented:
            total = np.array([0 + s for s in sums], dtype=object)
        for k, s in zip(nz.tolist(), np.asarray(total).reshape(-1)):
            res[k] = s
    return res


def segment_sum_packed(x, index_lists, layout, max_abs):
    """The per-bin sums of segment_sum as ONE PackedCiphertextBuffer (packed_buffer.py): one pai_segment_add call, then
    one pai_pack_ciphertexts call that folds layout.slots bin sums into each ciphertext, so the key holder decrypts
    len(index_lists) / slots ciphertexts; no per-bin object is built. `x` is a CiphertextBuffer, a PaillierArray or an
    object array of integer-valued ciphertexts with |value| <= max_abs (the caller's assertion); the buffer's bound is
    (longest bin) * ceil(max_abs * 16^exponent), OverflowError before any GPU call if it passes the slot. Empty bins
    decode as 0. Without a GPU the same runs on Python integers (small arrays only)."""
    from . import _runtime
    from .cipher_array import _encrypted_operand, pack
    from .cipher_buffer import CiphertextBuffer
    from .packed_buffer import _EMPTY_EXP, _fold, _ints, _slot_bound, _to_words
    if isinstance(x, CiphertextBuffer):
        pk, words, exps = x.public_key, x.words, x.exps
    else:
        A, pk = _encrypted_operand(x)
        if A is None:
            raise TypeError("segment_sum_packed needs a non-empty array of PaillierEncryptedNumber with one public key")
        words, exps, _ = pack(x, pk)
    lists = [np.asarray(i).reshape(-1) for i in index_lists]
    sizes = np.array([len(i) for i in lists], dtype=np.int64)
    bound = _slot_bound(layout, max_abs, int(sizes.max()) if sizes.size else 0)
    idx = np.concatenate(lists).astype(np.int64) if sizes.sum() else np.zeros(0, dtype=np.int64)
    idx = np.where(idx < 0, idx + exps.size, idx)
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if _runtime.gpu_available():
        out, oe = _runtime.context(pk).segment_add(words, exps, idx, seg_off)
    else:
        cts, nsq, sums, oe = _ints(words), pk.nsquare, [], []
        for s in range(len(lists)):
            members = idx[seg_off[s]:seg_off[s + 1]].tolist()
            E = max((int(exps[i]) for i in members), default=_EMPTY_EXP)
            acc = 1
            for i in members:
                acc = acc * pow(cts[i], 16 ** (E - int(exps[i])), nsq) % nsq
            sums.append(acc)
            oe.append(E)
        out, oe = _to_words(sums, words.shape[1]), np.array(oe, dtype=np.int32)
    return _fold(pk, out, np.ascontiguousarray(oe, dtype=np.int32), layout, bound, (len(lists),))


def _on_device(x) -> bool:
    from .device_buffer import DeviceCiphertextBuffer
    return isinstance(x, DeviceCiphertextBuffer)


def _histogram_operand(x, who: str):
    from .cipher_array import _encrypted_operand, pack
    from .cipher_buffer import CiphertextBuffer
    if isinstance(x, CiphertextBuffer):
        return x.public_key, x.words, x.exps
    if _on_device(x):
        return x.public_key, x.words, x._ex                 # device holders: the cells stay on the device
    A, pk = _encrypted_operand(x)
    if A is None:
        raise TypeError(f"{who} needs a non-empty array of PaillierEncryptedNumber with one public key")
    words, exps, _ = pack(x, pk)
    return pk, words, exps


def _histogram_cells(pk, words, exps, bins, n_bins, node, n_nodes, default_bin):
    """(words, exponents, counts, shape) of the histogram's cells: sparse bins (anything that offers .tocsr()) through
    pai_histogram_sparse, a numpy matrix through pai_histogram."""
    from .cipher_buffer import histogram_args, histogram_sparse_args, histogram_sparse_words, histogram_words, sparse_csr
    csr = sparse_csr(bins)
    if csr is not None:
        *args, shape = histogram_sparse_args(words.shape[0], csr, n_bins, node, n_nodes, default_bin)
        return histogram_sparse_words(pk, words, exps, *args, shape) + (shape,)
    b, nd, shape = histogram_args(words.shape[0], bins, n_bins, node, n_nodes)
    return histogram_words(pk, words, exps, b, shape[2], nd, shape[0]) + (shape,)


def histogram(x, bins, n_bins, node=None, n_nodes=1, default_bin=0):
    """Per-cell sums of the encrypted vector x (flat order) over the bin ids bins [N, F] (uint8 / uint16) and an optional
    node id per sample, all features at once: (PaillierArray of shape (n_nodes, F, n_bins), int64 counts of that shape)
    from ONE pai_histogram call, with no index list built (IV_FFS over every feature of a party, the (node, feature, bin)
    sums of gradient boosting). Cell [v, f, b] is the pure ``+`` reduction over the samples with node == v and
    bins[:, f] == b, without the ``0 +`` of Python's sum; a node id outside [0, n_nodes) and a bin id >= n_bins put the
    sample in no cell (of that feature). An empty cell is ciphertext 1 at exponent 0, an unobfuscated encryption of 0.
    Without a GPU the same runs on Python integers.
    Sparse bins (anything that offers .tocsr()) take ONE pai_histogram_sparse call over the stored entries; every entry
    that is not stored has bin default_bin (a scalar or one per feature), and the default cell is the node's total minus
    the feature's other stored entries (``T - S`` of the reference's operators, CiphertextBuffer.histogram)."""
    from .cipher_array import materialize
    if _on_device(x):
        return x.histogram(bins, n_bins, node=node, n_nodes=n_nodes, default_bin=default_bin)
    pk, words, exps = _histogram_operand(x, "histogram")
    out, oe, cnt, shape = _histogram_cells(pk, words, exps, bins, n_bins, node, n_nodes, default_bin)
    oe = np.where(cnt == 0, 0, oe).astype(np.int32)
    return materialize(pk, out, oe, shape, obfuscated=False), cnt.reshape(shape)


def histogram_packed(x, bins, n_bins, layout, max_abs, node=None, n_nodes=1, default_bin=0):
    """The cell sums of histogram as ONE PackedCiphertextBuffer of shape (n_nodes, F, n_bins): one pai_histogram call,
    then one pai_pack_ciphertexts call that folds layout.slots cell sums into each ciphertext; returns (buffer, counts).
    A DeviceCiphertextBuffer gives a resident packed buffer (histogram and cumsum return device buffers for one too).
    `x` holds integer-valued ciphertexts at the layout's exponent with |value| <= max_abs (the caller's assertion); the
    buffer's bound is counts.max() * ceil(max_abs * 16^exponent), OverflowError before the fold if it passes the slot.
    Empty cells decode as 0. Without a GPU the same runs on Python integers (small arrays only). Sparse bins and
    default_bin as in histogram; a default cell is a subset sum like any other, so the bound rule is the same."""
    from .packed_buffer import _fold, _slot_bound
    pk, words, exps = _histogram_operand(x, "histogram_packed")
    _slot_bound(layout, max_abs, 1)                         # a single value already has to fit
    out, oe, cnt, shape = _histogram_cells(pk, words, exps, bins, n_bins, node, n_nodes, default_bin)
    bound = _slot_bound(layout, max_abs, int(cnt.max()) if cnt.size else 0)
    if _on_device(x):
        oe = oe.download(np.int32, cnt.size)                # exponents only: the cells fold where they are
    return _fold(pk, out, np.ascontiguousarray(oe, dtype=np.int32), layout, bound, shape), cnt.reshape(shape)


def repack(buf, slots=None):
    """PackedCiphertextBuffer.repack: the values of a packed buffer (what histogram_packed, or a packed g/h buffer's
    histogram and cumsum, return) in fewer, fuller ciphertexts of `slots` slots (default: as many as the key holds), in
    ONE pai_repack call; after the last cumsum, before to_wire(be_secure=True)."""
    from .packed_buffer import PackedCiphertextBuffer
    if not isinstance(buf, PackedCiphertextBuffer):
        raise TypeError(f"unsupported operand {type(buf)} for repack")
    return buf.repack(slots)


def good_bad_calc(y: np.ndarray, index_lists):
    """HeteroBin.en_good_bad_calc (hetero_bin.py:27-36) on the GPU: good_s = sum(y[i]), bad_s = len(i) -
    good_s for every bin; returns the two numpy arrays the reference builds."""
    good = segment_sum(y, index_lists)
    lens = np.array([len(np.asarray(i).reshape(-1)) for i in index_lists], dtype=np.int64)
    enc = [k for k, g in enumerate(good) if not isinstance(g, (int, np.integer))]
    bad = [int(n) - g if isinstance(g, (int, np.integer)) else None for n, g in zip(lens, good)]
    if enc:
        objs = np.empty(len(enc), dtype=object)
        objs[:] = [good[k] for k in enc]
        neg = mul_plain(objs, -1)                            # len - g = len + (g * -1)  (encrypted_number.py:77-78)
        b = add_plain(neg, lens[enc])
        for k, v in zip(enc, np.asarray(b).reshape(-1)):
            bad[k] = v
    return np.array(good), np.array(bad)
