"""The prime search's edge inputs, the parts that need no GPU: tests/golden/prime_edges.json (tools/make_prime_edges.py)
states only what the host functions recompute -- width, primality, s, shape, factors, the liars with their exits --; the
argument refusals of pai_prime_test and pai_next_prime that return before any device call (csrc/engine_prime.hip); and
the device search's sieve (pai_debug_prime_sieve) against trial division at the start shapes of
tests/test_gpu_prime_edges.py's families E and F."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_prime_edges as G                                            # noqa: E402
from test_gpu_prime import _strong_test                                 # noqa: E402
from test_prime_cpu import _native_or_skip, _trial_division             # noqa: E402


@pytest.fixture(scope="module")
def records():
    with open(os.path.join(ROOT, "tests", "golden", "prime_edges.json")) as f:
        doc = json.load(f)
    assert doc["generator"] == "tools/make_prime_edges.py"
    return doc["records"]


def test_fixture_holds_what_the_gpu_tests_take(records):
    keys = list((r["family"], r["bits"], r.get("shape") or r.get("s"), r["prime"]) for r in records if r["family"] != "D")
    want = []
    for bits in (1024, 2048):
        lane = G.LIMB * G.LW[bits]
        want += [("A", bits, "above_half", True), ("A", bits, "below_top", True)]
        want += [("A", bits, sh, p) for sh in G.SHAPES[:4 if bits == 1024 else 2] for p in (True, False)]
        want += [("B", bits, s, p) for s in (28, lane, bits // 2) for p in (True, False)]
    assert sorted(map(str, keys)) == sorted(map(str, want))
    assert sorted((r["bits"], r["t"]) for r in records if r["family"] == "D") == [(1024, 1), (1024, 3), (2048, 1), (2048, 3)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "prime_edges.json")) < 64 << 10


@pytest.mark.parametrize("bits", [1024, 2048])
def test_fixture_width_primality_s_and_shape(bits, records):
    from flex.crypto.paillier import _bigint
    for r in (r for r in records if r["bits"] == bits):
        n = int(r["n"], 16)
        assert n.bit_length() == bits and n % 2 == 1
        assert _bigint.is_probable_prime(n) == r["prime"], r
        if "s" in r:
            assert G.trailing_zeros(n - 1) == r["s"]
        if r["family"] == "A" and r["shape"] in G.SHAPES:
            assert G.has_shape(n, bits, r["shape"])
        if r["family"] != "A" and not r["prime"]:
            assert G.no_small_factor(n)                        # a composite the search's sieve would let through
    named = {r["shape"]: int(r["n"], 16) for r in records if r["bits"] == bits and r["family"] == "A"}
    lo, hi = named["above_half"], named["below_top"]
    assert lo > 1 << (bits - 1) and not any(G.is_prime(c) for c in range((1 << (bits - 1)) + 1, lo, 2))
    assert hi < 1 << bits and not any(G.is_prime(c) for c in range(hi + 2, 1 << bits, 2))


@pytest.mark.parametrize("bits", [1024, 2048])
def test_fixture_liars_with_their_exits(bits, records):
    from flex.crypto.paillier import _bigint
    for r in (r for r in records if r["bits"] == bits and r["family"] == "D"):
        n, p, q, t = int(r["n"], 16), int(r["p"], 16), int(r["q"], 16), r["t"]
        assert n == p * q and _bigint.is_probable_prime(p) and _bigint.is_probable_prime(q)
        assert (p - 1) >> t << (t + 1) == q - 1 and ((p - 1) >> t) % 2 == 1
        assert r["scanned_below"] == G.LIAR_SCAN[bits] and r["scanned_high_to"] >= 1 << 31
        span = list(range(r["scanned_below"])) + list(range(1 << 31, r["scanned_high_to"] + 1))
        got = [[a, how] for a, (ok, how) in ((a, _strong_test(n, a)) for a in span) if ok]
        assert got == r["liars"]
        assert sum(a >= 1 << 31 for a, _ in got) == G.LIAR_HIGH and got[-1][0] == r["scanned_high_to"]
        assert [1, "one"] in got and not any(a == 0 for a, _ in got)


NO_DEVICE = 10 ** 6      # a device number no machine has: a call that got as far as the device would fail on that, not on
                         # its arguments


def test_prime_test_refuses_before_any_device_call():
    _native = _native_or_skip()
    p = G.prime_above_half(256)
    for cands, bits, bases, why in (([p - 1], 256, [3], "odd with bit"),            # even
                                    ([p, p + 1], 256, [3], "odd with bit"),         # the second one even
                                    ([p >> 1 | 1], 256, [3], "odd with bit"),       # 255 bits
                                    ([p], 768, [3], "bad arguments"),               # not a size the kernel is built for
                                    ([p], 256, [], "bad arguments")):               # no bases
        with pytest.raises(_native.NativeError, match="pai_prime_test: .*" + why):
            _native.prime_test(cands, bits, bases, device=NO_DEVICE)


def test_next_prime_refuses_before_any_device_call():
    _native = _native_or_skip()
    x = 1 << 255 | 12345
    for starts, bits, window, why in (([x >> 1], 256, 0, "must have bit"),          # bit 255 not set
                                      ([x, x >> 1], 256, 0, "must have bit"),
                                      ([x] * 4097, 256, 0, "bad arguments"),
                                      ([x], 256, (1 << 24) + 1, "bad arguments"),
                                      ([x], 768, 0, "bad arguments")):
        with pytest.raises(_native.NativeError, match="pai_next_prime: .*" + why):
            _native.next_prime_batch(starts, bits, window=window, device=NO_DEVICE)


# the sieve at the start shapes of the GPU module's families E and F
def _ones_start(bits, L):
    import random
    hb = bits - L
    hi = random.Random(5000 + bits + L).getrandbits(hb) | 1 << (hb - 1)
    if hi == (1 << hb) - 1:
        hi -= 1
    return hi << L | (1 << L) - 1


# trial division is what costs here: the default window, 4 * bits, up to 1024 bits only
@pytest.mark.parametrize("bits,window", [(256, 64), (256, 0), (512, 64), (512, 0), (1024, 64), (1024, 0), (2048, 64)])
def test_sieve_at_starts_of_all_ones(bits, window):
    _native = _native_or_skip()
    lane = G.LIMB * G.LW[bits]
    for L in sorted({28, 56, lane, 2 * lane, bits - 2}):
        x = _ones_start(bits, L)
        assert x.bit_length() == bits and (x + 2) >> L == (x >> L) + 1
        want = _trial_division(x, window or 4 * bits)
        assert _native.prime_sieve(x, bits, window) == want, (bits, L)
        assert all(off % 2 == 0 for off in want) and (want or window)
    zero = (_ones_start(bits, 2 * lane) >> 2 * lane) << 2 * lane
    want = _trial_division(zero, window or 4 * bits)
    assert zero % 2 == 0 and want and want[0] % 2 == 1 and _native.prime_sieve(zero, bits, window) == want


@pytest.mark.parametrize("long_gap", [False, True])
@pytest.mark.parametrize("bits", [256, 512])
def test_sieve_keeps_the_pseudoprime(bits, long_gap):
    """Family F's starts, two below a composite with large factors that passes base 3: offset 2 survives the sieve, so
    the device's pass 1 meets it."""
    _native = _native_or_skip()
    n = G.base3_pseudoprime(bits, long_gap, 9500 + bits)
    x = n - 2
    assert x.bit_length() == bits and _strong_test(n, 3)[0] and not G.is_prime(n)
    for window in (64, 0):
        got = _native.prime_sieve(x, bits, window)
        assert got == _trial_division(x, window or 4 * bits) and got[0] == 2
