"""pai_take_idx_dev and pai_segment_add_idx_dev (index lists in device memory) against the host-list entry points
pai_take_dev and pai_segment_add_dev on the same lists, bit for bit, at 64-, 65- and 256-word rows; the oracle's + chain
on a few segments; and the device-side check: bad lists leave d_bad set, the outputs untouched and the context usable."""
import hashlib

import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
EMPTY = -(1 << 31)
I64_MIN = -(1 << 63)
N_TAKE, N_SEG = 300, 600
SEG_LENS = (0, 1, 15, 16, 17, 255, 256, 257)      # one, two and three levels at 16 members per part


def _native():
    from flex.crypto.paillier import _native as N
    return N


def _golden_key(golden, nb):
    k = golden["keys"][str(nb)]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _keys(golden, name):
    if name == "K1035":                                # ct_words 65: k_take moves rows word by word
        from test_gpu_ops_sizes import _make_key
        return _make_key("K1035", None)
    return _golden_key(golden, int(name[1:]))


class Side(object):
    """A context of one key with N_SEG (64 at 4096 bits) encrypted float64 values of mixed sign and magnitude on the
    device."""

    def __init__(self, golden, name):
        N = _native()
        n = 64 if name == "K4096" else N_SEG
        self.key = _keys(golden, name)
        self.ctx = N.Context(self.key.n, 0)
        self.W = self.ctx.ct_words
        rng = np.random.default_rng(len(name) + self.W)
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
        rk = hashlib.sha256(b"didx-" + name.encode()).digest()
        self.words, self.exps, st = self.ctx.encrypt(x, obf_mode=N.PAI_OBF_RNG, rng_key=rk, index_base=0)
        assert not st.any() and np.unique(self.exps).size > 3 and (x < 0).any()
        self.d_ct, self.d_ex = N.device_upload(self.words), N.device_upload(self.exps)

    # ---- the code under test, on uploaded lists; returns (words, exponents, d_bad) of a pre-filled output
    def take_idx(self, idx, n, allow_empty, fill=None):
        N = _native()
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        M = idx.size
        d_idx = N.device_upload(idx) if M else None
        out, oe, bad = self._outputs(M, fill)
        self.ctx.take_idx_dev(self.d_ct.ptr, self.d_ex.ptr, n, d_idx.ptr if M else None, M, allow_empty, out.ptr, oe.ptr,
                              bad.ptr)
        return self._down(out, oe, bad, M)

    def seg_idx(self, idx, off, n, fill=None, total=None):
        N = _native()
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        off = np.ascontiguousarray(off, dtype=np.int64)
        nseg = off.size - 1
        d_idx = N.device_upload(idx) if idx.size else None
        d_off = N.device_upload(off)
        out, oe, bad = self._outputs(nseg, fill)
        self.ctx.segment_add_idx_dev(self.d_ct.ptr, self.d_ex.ptr, n, d_idx.ptr if idx.size else None,
                                     idx.size if total is None else total, d_off.ptr, nseg, out.ptr, oe.ptr, bad.ptr)
        return self._down(out, oe, bad, nseg)

    # ---- the parent's entry points on the same host lists
    def take_host(self, idx, n):
        N = _native()
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out, oe, _ = self._outputs(idx.size, None)
        self.ctx.take_dev(self.d_ct.ptr, self.d_ex.ptr, n, idx, out.ptr, oe.ptr)
        return out.download(np.uint32, idx.size * self.W).reshape(idx.size, self.W), oe.download(np.int32, idx.size)

    def seg_host(self, idx, off, n):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        off = np.ascontiguousarray(off, dtype=np.int64)
        nseg = off.size - 1
        out, oe, _ = self._outputs(nseg, None)
        self.ctx.dev_call("pai_segment_add_dev", self.d_ct.ptr, self.d_ex.ptr, n, idx.ctypes.data if idx.size else None,
                          off.ctypes.data, nseg, out.ptr, oe.ptr)
        return out.download(np.uint32, nseg * self.W).reshape(nseg, self.W), oe.download(np.int32, nseg)

    def _outputs(self, rows, fill):
        N = _native()
        if fill is None:
            return N.DeviceMem(rows * self.W * 4, 0), N.DeviceMem(rows * 4, 0), N.DeviceMem(16, 0)
        return (N.device_upload(np.full((rows, self.W), fill, dtype=np.uint32)),
                N.device_upload(np.full(rows, 77, dtype=np.int32)), N.device_upload(np.array([5, 6], dtype=np.int64)))

    def _down(self, out, oe, bad, rows):
        return (out.download(np.uint32, rows * self.W).reshape(rows, self.W), oe.download(np.int32, rows),
                bad.download(np.int64, 2))


@pytest.fixture(scope="module")
def sides(golden):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Side(golden, name)
        return made[name]
    yield get
    for s in made.values():
        s.ctx.close()


def _seg_lists(seed, lens, n):
    """Index lists with repeats inside and across segments."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, n, int(off[-1])).astype(np.int64)
    if idx.size > 40:
        idx[5:9] = idx[4]                      # repeated inside a segment
        idx[-20:] = idx[20:40]                 # shared between segments
    return idx, off


# ------------------------------------------------------------------------------------------ take
@pytest.mark.parametrize("name", ["K1024", "K1035"])
def test_take_matches_the_host_index_call(sides, name):
    s = sides(name)
    rng = np.random.default_rng(3)
    one = np.zeros(s.W, dtype=np.uint32)
    one[0] = 1
    for M in (0, 1, 255, 256, 257):
        idx = rng.integers(0, N_TAKE, M).astype(np.int64)
        if M > 10:
            idx[3:7] = idx[2]                  # repeated entries
            idx[-1] = N_TAKE - 1
            idx[0] = 0
        for allow_empty in (0, 1):
            if allow_empty and M:
                idx = idx.copy()
                idx[::5] = -1
            got, ge, bad = s.take_idx(idx, N_TAKE, allow_empty)
            assert bad.tolist() == [-1, -1], (M, allow_empty)
            hw, he = s.take_host(idx, N_TAKE)
            assert np.array_equal(got, hw) and np.array_equal(ge, he), (M, allow_empty)
            want = np.where((idx >= 0)[:, None], s.words[np.maximum(idx, 0)], one[None, :]).reshape(M, s.W)
            assert np.array_equal(got, want), (M, allow_empty)
            assert np.array_equal(ge, np.where(idx >= 0, s.exps[np.maximum(idx, 0)], EMPTY))


# ------------------------------------------------------------------------------------------ segment sums
def _oracle_segment(s, idx, off, j):
    mem = idx[off[j]:off[j + 1]]
    if mem.size == 0:
        return 1, EMPTY
    cts = _native().words_to_ints(s.words[mem])
    return O.add_k(cts, [int(e) for e in s.exps[mem]], s.key)


@pytest.mark.parametrize("name", ["K1024", "K1035"])
def test_segment_sums_match_the_host_list_call(sides, name):
    N = _native()
    s = sides(name)
    idx, off = _seg_lists(17, SEG_LENS, N_SEG)
    got, ge, bad = s.seg_idx(idx, off, N_SEG)
    assert bad.tolist() == [-1, -1]
    hw, he = s.seg_host(idx, off, N_SEG)
    assert np.array_equal(ge, he) and np.array_equal(got, hw)
    assert ge[0] == EMPTY and got[0, 0] == 1 and not got[0, 1:].any()
    ints = N.words_to_ints(got)
    for j in (0, 1, 4, 7):                     # lengths 0, 1, 17 and 257
        assert (ints[j], int(ge[j])) == _oracle_segment(s, idx, off, j), j


@pytest.mark.parametrize("lens", [(300,), (0, 0, 0), (6,) * 100, (0, 40, 0, 1, 0)],
                         ids=["one-segment", "all-empty", "short-segments-pass-through", "empty-between"])
def test_segment_special_shapes(sides, lens):
    """(6,) * 100: 600 entries make the device plan three levels where the host list needs one; the finished segments
    pass through the other two unchanged."""
    s = sides("K1024")
    idx, off = _seg_lists(len(lens), lens, N_SEG)
    got, ge, bad = s.seg_idx(idx, off, N_SEG)
    hw, he = s.seg_host(idx, off, N_SEG)
    assert bad.tolist() == [-1, -1]
    assert np.array_equal(ge, he) and np.array_equal(got, hw)
    if not idx.size:                           # total = 0: no index is needed, and none is read
        assert (ge == EMPTY).all() and (got[:, 0] == 1).all() and not got[:, 1:].any()
        mark = 0xA5A5A5A5
        got2, ge2, bad2 = s.seg_idx(np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), N_SEG, fill=mark)
        assert bad2.tolist() == [-1, -1] and got2.shape == (0, s.W)       # nseg = 0


def test_eight_lane_groups(sides):
    """The 4096-bit golden key: 256-word rows through k_add<8>."""
    s = sides("K4096")
    idx, off = _seg_lists(5, (0, 1, 17, 40), 64)
    got, ge, bad = s.seg_idx(idx, off, 64)
    hw, he = s.seg_host(idx, off, 64)
    assert bad.tolist() == [-1, -1] and np.array_equal(ge, he) and np.array_equal(got, hw)
    ints = _native().words_to_ints(got)
    assert (ints[2], int(ge[2])) == _oracle_segment(s, idx, off, 2)
    tidx = np.array([63, -1, 0, 0, 17], dtype=np.int64)
    tw, te, tbad = s.take_idx(tidx, 64, 1)
    hw, he = s.take_host(tidx, 64)
    assert tbad.tolist() == [-1, -1] and np.array_equal(tw, hw) and np.array_equal(te, he)


# ------------------------------------------------------------------------------------------ bad lists
MARK = 0xA5A5A5A5
BAD_VALUES = {"N": None, "minus1": -1, "minus2": -2, "int64min": I64_MIN}
POSITIONS = {"first": 0, "last": -1, "past256": 270}


def _untouched(got, ge):
    return (got == MARK).all() and (ge == 77).all()


@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("what", list(BAD_VALUES))
def test_bad_index_values_shut_the_gate(sides, what, where):
    """No kernel behind the check reads through the index once a word of d_bad is set: the sentinel survives, the call
    returns PAI_OK, d_bad names the smallest offender, and the context serves a valid call afterwards."""
    s = sides("K1024")
    value = N_TAKE if BAD_VALUES[what] is None else BAD_VALUES[what]
    rng = np.random.default_rng(9)
    idx = rng.integers(0, N_TAKE, 300).astype(np.int64)
    pos = POSITIONS[where] % idx.size
    idx[pos] = value
    got, ge, bad = s.take_idx(idx, N_TAKE, 0, fill=MARK)
    assert bad.tolist() == [pos, -1] and _untouched(got, ge)
    if value != -1:                            # -1 is an entry of its own with allow_empty
        got, ge, bad = s.take_idx(idx, N_TAKE, 1, fill=MARK)
        assert bad.tolist() == [pos, -1] and _untouched(got, ge)
    off = np.array([0, 1, 17, 280, 280, 300], dtype=np.int64)
    got, ge, bad = s.seg_idx(idx, off, N_TAKE, fill=MARK)
    assert bad.tolist() == [pos, -1] and _untouched(got, ge)
    if pos + 7 < idx.size:                     # a second offender further on: the smallest position is named
        idx[pos + 7] = -5
        assert s.take_idx(idx, N_TAKE, 0, fill=MARK)[2].tolist() == [pos, -1]
        assert s.seg_idx(idx, off, N_TAKE, fill=MARK)[2].tolist() == [pos, -1]
    # the context after the refused lists
    idx[idx < 0] = 0
    idx[idx >= N_TAKE] = 0
    got, ge, bad = s.take_idx(idx, N_TAKE, 0, fill=MARK)
    assert bad.tolist() == [-1, -1] and np.array_equal(got, s.words[idx]) and np.array_equal(ge, s.exps[idx])
    got, ge, bad = s.seg_idx(idx, off, N_TAKE, fill=MARK)
    hw, he = s.seg_host(idx, off, N_TAKE)
    assert bad.tolist() == [-1, -1] and np.array_equal(got, hw) and np.array_equal(ge, he)


@pytest.mark.parametrize("case", ["first-offset-1", "decreasing", "end-below-total", "end-above-total", "both-lists"])
def test_bad_offsets_shut_the_gate(sides, case):
    s = sides("K1024")
    idx = np.random.default_rng(4).integers(0, N_SEG, 300).astype(np.int64)
    good = np.array([0, 1, 17, 280, 280, 300], dtype=np.int64)
    off, total, want = good.copy(), None, None
    if case == "first-offset-1":
        off[0], want = 1, [-1, 0]
    elif case == "decreasing":
        off[3], want = 16, [-1, 3]             # [0, 1, 17, 16, 280, 300]: position 3 is below its neighbour
    elif case == "end-below-total":
        off[5], want = 299, [-1, 5]
    elif case == "end-above-total":
        total, want = 299, [-1, 5]             # the list holds 300 entries; the caller says 299
    else:
        off[0], want = 1, [44, 0]
        idx[44] = N_SEG
        idx[200] = -1
    got, ge, bad = s.seg_idx(idx, off, N_SEG, fill=MARK, total=total)
    assert bad.tolist() == want and _untouched(got, ge)
    idx[idx < 0] = 0
    idx[idx >= N_SEG] = 0
    got, ge, bad = s.seg_idx(idx, good, N_SEG, fill=MARK)
    hw, he = s.seg_host(idx, good, N_SEG)
    assert bad.tolist() == [-1, -1] and np.array_equal(got, hw) and np.array_equal(ge, he)


def test_what_the_host_can_see_is_refused_before_any_launch(sides):
    N = _native()
    s = sides("K1024")
    idx = N.device_upload(np.arange(4, dtype=np.int64))
    off = N.device_upload(np.array([0, 4], dtype=np.int64))
    out, oe, bad = s._outputs(4, MARK)
    c, e = s.d_ct.ptr, s.d_ex.ptr
    with pytest.raises(N.NativeError, match="null pointer"):
        s.ctx.take_idx_dev(c, e, N_SEG, idx.ptr, 4, 0, out.ptr, oe.ptr, None)
    with pytest.raises(N.NativeError, match="null pointer"):
        s.ctx.take_idx_dev(c, e, N_SEG, None, 4, 0, out.ptr, oe.ptr, bad.ptr)
    with pytest.raises(N.NativeError, match="overlaps"):
        s.ctx.take_idx_dev(c, e, N_SEG, idx.ptr, 4, 0, s.d_ct.at(8 * s.W * 4), oe.ptr, bad.ptr)
    with pytest.raises(N.NativeError, match="too many rows"):
        s.ctx.take_idx_dev(c, e, N_SEG, idx.ptr, 1 << 40, 0, out.ptr, oe.ptr, bad.ptr)
    with pytest.raises(N.NativeError, match="null pointer"):
        s.ctx.segment_add_idx_dev(c, e, N_SEG, idx.ptr, 4, None, 1, out.ptr, oe.ptr, bad.ptr)
    with pytest.raises(N.NativeError, match="null pointer"):
        s.ctx.segment_add_idx_dev(c, e, N_SEG, None, 4, off.ptr, 1, out.ptr, oe.ptr, bad.ptr)
    with pytest.raises(N.NativeError, match="overlaps"):
        s.ctx.segment_add_idx_dev(c, e, N_SEG, idx.ptr, 4, off.ptr, 1, out.ptr, s.d_ex.at(16), bad.ptr)
    with pytest.raises(N.NativeError, match="too many rows"):
        s.ctx.segment_add_idx_dev(c, e, N_SEG, idx.ptr, 1 << 40, off.ptr, 1, out.ptr, oe.ptr, bad.ptr)
    got, ge, b = s._down(out, oe, bad, 4)
    assert _untouched(got, ge) and b.tolist() == [5, 6]                   # not even d_bad was written
