"""pai_segment_dot_idx_dev (index lists, offsets and weights in device memory; csrc/kernels_sdi.hpp) against the oracle's
Python integers (mul_scalar per gathered entry, add_k per segment) and against pai_segment_dot_dev on the same lists, bit
for bit, at lane groups of 2, 4 and 8 and at 65-word rows; the device-side gates; and DeviceCiphertextBuffer.segment_dot
over three DeviceArrays."""
import numpy as np
import pytest

from oracle import paillier_oracle as O

pytestmark = pytest.mark.gpu
EMPTY = -(1 << 31)
LENS = (0, 1, 2, 15, 16, 17, 33, 0)          # the row seams of 16 and a second tree level (84 entries)
DTYPES = {"f32": np.float32, "f64": np.float64, "i64": np.int64}


def _native():
    from flex.crypto.paillier import _native as N
    return N


def _key(golden, name):
    if name == "K1035":                       # seeded; ct_words 65; the group's limb bits equal 2 nb + 2
        seed = 1
        while True:                           # step the seed until n has exactly 1035 bits
            p, q = O.getprimeover(518, seed=seed), O.getprimeover(517, seed=seed + 1000)
            if p != q and (p * q).bit_length() == 1035:
                return O.Key(p * q, p, q)
            seed += 1
    k = golden["keys"][name[1:]]
    return O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))


def _lists(dtype, n):
    """One list over n ciphertexts: (index, offsets, weights). Segment 3 (15 entries) is all negative, segment 4 (16) all
    positive, the others mix signs inside a row; repeats inside a row and across segments; zeros, -0.0 and one NaN."""
    rng = np.random.default_rng(n)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    total = int(off[-1])
    idx = rng.integers(0, n, total).astype(np.int64)
    idx[off[5] + 1] = idx[off[5]] = idx[off[3]] = idx[off[6] + 20]       # one ciphertext twice in a row and in 3 segments
    sign = np.where(rng.random(total) < 0.5, -1.0, 1.0)
    sign[off[3]:off[4]], sign[off[4]:off[5]] = -1.0, 1.0
    if dtype == np.int64:
        w = (sign * rng.integers(1, 1000, total)).astype(np.int64)
        w[off[6]:off[6] + 5] = (1, -1, 1 << 62, 0, -(1 << 62))
    else:
        w = (sign * 10.0 ** rng.uniform(-8, 8, total)).astype(dtype)
        w[off[6]:off[6] + 4] = (0.0, -0.0, np.nan, 1.0)
        w[off[2]] = 0.0                                                  # a stored zero in a segment of two
    return idx, off, w


class Side(object):
    """A public-key context with n random residues mod n^2 at exponents spread over 0 .. 24 on the device."""

    def __init__(self, golden, name):
        N = _native()
        self.key, self.n = _key(golden, name), 8 if name == "K4096" else 24
        self.ctx = N.Context(self.key.n, 0)
        self.W = self.ctx.ct_words
        rng = np.random.default_rng(self.W)
        self.ints = [int.from_bytes(rng.bytes(4 * self.W + 8), "little") % self.key.nsquare for _ in range(self.n)]
        self.exps = (np.arange(self.n) * 24 // (self.n - 1)).astype(np.int32)
        self.d_ex = N.device_upload(self.exps)

    def run(self, idx, off, w, ints=None, host=False):
        """(words, exponents, statuses, check words) of pre-filled outputs; host=True: pai_segment_dot_dev."""
        N = _native()
        nseg, total = off.size - 1, idx.size
        d_ct = N.device_upload(N.ints_to_words(self.ints if ints is None else ints, self.W))
        d_x = N.device_upload(w)
        out = N.device_upload(np.full((nseg, self.W), 0xABCD0123, dtype=np.uint32))
        oe, st = N.device_upload(np.full(nseg, 77, dtype=np.int32)), N.device_upload(np.full(total, 66, dtype=np.int32))
        bad = N.device_upload(np.array([5, 6, 7, 8], dtype=np.int64))
        if host:
            self.ctx.dev_call("pai_segment_dot_dev", d_ct.ptr, self.d_ex.ptr, self.n, idx.ctypes.data, off.ctypes.data, nseg,
                              N.scalar_dtype(w), d_x.ptr, out.ptr, oe.ptr, st.ptr)
        else:
            d_idx, d_off = N.device_upload(idx), N.device_upload(off)
            self.ctx.segment_dot_idx_dev(d_ct.ptr, self.d_ex.ptr, self.n, d_idx.ptr, total, d_off.ptr, nseg,
                                         N.scalar_dtype(w), d_x.ptr, out.ptr, oe.ptr, st.ptr, bad.ptr)
        return (out.download(np.uint32, nseg * self.W).reshape(nseg, self.W), oe.download(np.int32, nseg),
                st.download(np.int32, total), bad.download(np.int64, 4))


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


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", ["K1024", "K1035", "K2048", "K4096"])
def test_parity_with_oracle_and_host_lists(sides, name, dtype):
    N, s = _native(), sides(name)
    idx, off, w = _lists(DTYPES[dtype], s.n)
    words, exps, st, bad = s.run(idx, off, w)
    nan = np.flatnonzero(w != w)
    assert list(bad) == [-1, -1, -1, nan[0] if nan.size else -1]
    assert np.array_equal(st, np.where(w != w, N.EL_ENC_RANGE, 0))
    got = N.words_to_ints(words)
    for g in range(len(LENS)):
        terms = [(1, int(s.exps[idx[t]])) if w[t] != w[t] else
                 O.mul_scalar(s.ints[idx[t]], int(s.exps[idx[t]]), w[t].item(), s.key) for t in range(off[g], off[g + 1])]
        want = O.add_k([c for c, _ in terms], [e for _, e in terms], s.key) if terms else (1, EMPTY)
        assert (got[g], int(exps[g])) == want, (name, dtype, g)
    hw, he, hs, _ = s.run(idx, off, w, host=True)
    assert np.array_equal(words, hw) and np.array_equal(exps, he) and np.array_equal(st, hs)


@pytest.mark.parametrize("case,word", [("index_N", 0), ("index_neg", 0), ("offset_decreasing", 1), ("offset_end", 1),
                                       ("noinv", 2)])
def test_gates_leave_outputs_untouched(sides, case, word):
    s = sides("K1024")
    idx, off, w = _lists(np.float64, s.n)
    ints, t = list(s.ints), int(off[6]) + 7
    if case == "index_N":
        idx[t] = s.n
    elif case == "index_neg":
        idx[t] = -1
    elif case == "offset_decreasing":
        off[3] = off[2] - 1
    elif case == "offset_end":
        off[-1] += 1
    else:
        ints[idx[t]], w[idx == idx[t]] = s.key.n, -1.5
    words, exps, st, bad = s.run(idx, off, w, ints)
    want = {"index_N": t, "index_neg": t, "offset_decreasing": 3, "offset_end": len(LENS), "noinv": 1}[case]
    assert bad[word] == want and all(bad[k] == -1 for k in range(3) if k != word)
    assert (words == 0xABCD0123).all() and (exps == 77).all() and (st == 66).all()
    if case == "noinv":                      # the same list with the weight made positive succeeds
        w[idx == idx[t]] = 1.5
        words, exps, st, bad = s.run(idx, off, w, ints)
        hw, he, hs, _ = s.run(idx, off, w, ints, host=True)
        assert list(bad[:3]) == [-1, -1, -1] and np.array_equal(words, hw) and np.array_equal(exps, he)
        assert np.array_equal(st, hs)


def _buffer(s):
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.keypair import PaillierPublicKey
    return CiphertextBuffer(PaillierPublicKey(s.key.n), _native().ints_to_words(s.ints, s.W), s.exps)


def test_python_route_matches_host_lists_and_uploads_nothing(sides):
    from flex.crypto.paillier.device_buffer import device_array
    N, s = _native(), sides("K2048")
    idx, off, w = _lists(np.float64, s.n)
    w[w != w] = 3.25
    dev = _buffer(s).to_device()
    full, packed = off, off[np.concatenate([[True], np.diff(off) > 0])]       # the same entries without the empty segments
    for o in (full, packed):
        want = dev.segment_dot(idx, o, w).to_host()
        d_idx, d_off, d_w = device_array(idx), device_array(o), device_array(w)
        up = N.dev_io_stats()[0]
        got = dev.segment_dot(d_idx, d_off, d_w)
        # no list byte goes up; an empty segment's exponent is rewritten to 0 on the host, so the nseg exponents do
        assert N.dev_io_stats()[0] - up == (4 * (o.size - 1) if o is full else 0)
        got = got.to_host()
        assert got.shape == want.shape and np.array_equal(got.words, want.words) and np.array_equal(got.exps, want.exps)


@pytest.mark.parametrize("case,exc", [("offsets", ValueError), ("index", IndexError), ("nan", ValueError),
                                      ("noinv", ZeroDivisionError), ("mixed", TypeError)])
def test_python_route_raises_what_the_host_lists_raise(sides, case, exc):
    from flex.crypto.paillier.device_buffer import device_array
    s = sides("K1024")
    idx, off, w = _lists(np.float64, s.n)
    w[w != w] = 3.25
    buf = _buffer(s)
    if case == "offsets":
        off[3] = off[2] - 1
    elif case == "index":
        idx[5] = s.n
    elif case == "nan":
        w[9] = np.nan
    elif case == "noinv":
        buf.words[idx[9]], w[9] = _native().ints_to_words([s.key.n], s.W)[0], -2.0
    ops = [device_array(idx), device_array(off), w if case == "mixed" else device_array(w)]
    with pytest.raises(exc, match="weights" if case == "mixed" else None):
        buf.to_device().segment_dot(*ops)
