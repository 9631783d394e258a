"""The prime search at the edges of its arithmetic (csrc/kernels_prime.hpp k_mr_w, csrc/engine_prime.hip): inputs that
random candidates never give, each family with a precondition test that shows on the CPU that its inputs have the
property they are there for. Every verdict is compared with test_gpu_prime._strong_test on Python integers, every search
with _bigint.next_prime; candidates treated as primes are primes to oracle.paillier_oracle._is_probable_prime as well.

  A  the modulus' shape: 2^(BITS-1) + 1, the primes next to 2^(BITS-1) and 2^BITS, 2^BITS - 1, runs of ones and of
     zeros over two whole lanes, limb 0 = 2^28 - 1 and = 1; 3 and 5 bases, so that a wave straddles two candidates
  B  n = d 2^s + 1 with s across a limb, a lane, half the width and up to BITS - 1; s = 1 next to s >= 100 in one wave
  C  bases 0, 1, 2, 4, 2^16, 2^31, 2^31 + 1, 2^32 - 1 and random 32-bit ones, 2-bit and 32-bit bases in one wave
  D  strong liars of (2^t r + 1)(2^(t+1) r + 1): composites that pass by each of the three passing exits
  E  starts whose low L bits are all ones: the carry of x + offset over limbs and lanes (next_prime_batch)
  F  a start two below a composite that passes base 3: pass 2 rejects, and a 64-wide window refills
  G  one batch of starts at different stages, one of them handed back
  H  1025 x 4096 work items: the second trip of the kernel's grid-stride loop
  I  _bigint.next_primes' per-start host fallback and its counters

1024- and 2048-bit inputs of A, B and D come from tests/golden/prime_edges.json (tools/make_prime_edges.py), the rest is
built here, seeded, by that tool's generators.

59 cases (20 of them preconditions on the CPU); the whole module takes 25.8 s on an MI355X box, nearly all of it the host's
Python pow on the 1024- and 2048-bit references (the slowest case, A's precondition at 2048 bits, 3.7 s). H's 4.2 M work
items -- a 50 MB upload, the kernel, a 4.2 MB readback and the comparison of every entry -- take 0.13 s.
"""
import os
import random
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_prime_edges as G                                            # noqa: E402
from test_gpu_prime import _bases, _built_prime, _seeded_start, _strong_test   # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (256, 512, 1024, 2048)
LW, LIMB = G.LW, G.LIMB
PASSING = {"one", "minus_one", "squared"}


# ---------------------------------------------------------------- what the comparisons read back
def _device_matrix(cands, bits, bases):
    from flex.crypto.paillier import _native
    return _native.prime_test(cands, bits, bases)


def _device_search(starts, bits, window=0):
    from flex.crypto.paillier import _native
    return _native.next_prime_batch(starts, bits, window=window)


def _host_matrix(cands, bases):
    return np.array([[_strong_test(n, int(a))[0] for a in bases] for n in cands], dtype=np.uint8)


def _assert_matrix(got, want, cands, bases, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size:
        i, j = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} verdicts differ, the first at candidate {i} "
                             f"({hex(cands[i % len(cands)])}), base index {j} (base {int(bases[j % len(bases)])}): device "
                             f"{int(got[i, j])}, host {int(want[i, j])}")


def _assert_search(got, want, starts, what):
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (f"{what}: {len(bad)} of {len(want)} primes differ, the first at start {bad[0]} ({hex(starts[bad[0]])}): "
                     f"device {got[bad[0]] and hex(got[bad[0]])}, host {hex(want[bad[0]])}")


@lru_cache(maxsize=None)
def _prime_to_both(n):
    from flex.crypto.paillier import _bigint
    from oracle import paillier_oracle as O
    p = _bigint.is_probable_prime(n)
    assert O._is_probable_prime(n) == p, hex(n)
    return p


def _assert_primes_agree(cands):
    """Both restatements of the reference's primality test give the same answer; returns the primes."""
    return [n for n in cands if _prime_to_both(n)]


@pytest.fixture(scope="module")
def edges():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prime_edges.json")) as f:
        recs = json.load(f)["records"]
    for r in recs:
        for k in ("n", "p", "q"):
            if k in r:
                r[k] = int(r[k], 16)
    return recs


def _recs(edges, family, bits):
    return [r for r in edges if (r["family"], r["bits"]) == (family, bits)]


# ---------------------------------------------------------------- A: the shape of the modulus
@lru_cache(maxsize=None)
def _built_a(bits):
    """256 and 512 bits: [(shape, n)] as the fixture holds them for the larger widths"""
    named = [("above_half", G.prime_above_half(bits)), ("below_top", G.prime_below_top(bits))]
    for k, sh in enumerate(G.SHAPES):
        p, c = G.shaped_pair(bits, sh, 7000 + bits + k)
        named += [(sh, p), (sh, c)]
    return named


@pytest.fixture(scope="module")
def family_a(edges):
    """bits -> [(name, n)]; the first four are 2^(BITS-1) + 1, the primes next to 2^(BITS-1) and 2^BITS, 2^BITS - 1"""
    out = {}
    for bits in WIDTHS:
        named = _built_a(bits) if bits <= 512 else [(r["shape"], r["n"]) for r in _recs(edges, "A", bits)]
        assert [name for name, _ in named[:2]] == ["above_half", "below_top"]
        out[bits] = [("2^(BITS-1)+1", (1 << (bits - 1)) + 1)] + named[:2] + [("2^BITS-1", (1 << bits) - 1)] + named[2:]
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_shapes_are_what_they_claim(bits, family_a):
    named = family_a[bits]
    cands = [n for _, n in named]
    assert all(n % 2 == 1 and n.bit_length() == bits for n in cands)
    primes = _assert_primes_agree(cands)
    assert len(primes) >= 2 and len(cands) - len(primes) >= 2
    lo, hi = cands[1], cands[2]
    assert lo in primes and hi in primes
    # nothing but zero lanes between the top bit and the low limb; nothing but ones above the low limb
    assert 0 < lo - (1 << (bits - 1)) < 1 << LIMB and 0 < (1 << bits) - hi < 1 << LIMB
    if bits <= 512:                                             # the smallest and the largest such (the fixture's: CPU test)
        assert not any(G.is_prime(c) for c in range((1 << (bits - 1)) + 1, lo, 2))
        assert not any(G.is_prime(c) for c in range(hi + 2, 1 << bits, 2))
    for sh in G.SHAPES[:2 if bits == 2048 else 4]:              # limb 0 matters to m' alone: not repeated at 2048 bits
        mine = [n for name, n in named if name == sh]
        assert len(mine) == 2 and all(G.has_shape(n, bits, sh) for n in mine)
        assert [n in primes for n in mine] == [True, False]
    assert len(cands) == (8 if bits == 2048 else 12)
    lane = LIMB * LW[bits]
    assert 3 * lane < bits                                      # the runs sit below the top bit: whole lanes 1 and 2


@pytest.mark.parametrize("nbases", [3, 5])
@pytest.mark.parametrize("bits", WIDTHS)
def test_a_verdicts_equal_host(bits, nbases, family_a):
    cands = [n for _, n in family_a[bits]]
    bases = _bases()[:3] if nbases == 3 else _bases()[5:10]
    assert len(bases) % 4 and len(cands) * len(bases) > 8
    _assert_matrix(_device_matrix(cands, bits, bases), _host_matrix(cands, bases), cands, bases, f"A {bits}/{nbases}")


# ---------------------------------------------------------------- B: deep and seam-crossing s
def _s_list(bits):
    lane = LIMB * LW[bits]
    return sorted({27, 28, 29, 55, 56, 57, lane - 1, lane, lane + 1, bits // 2, bits - 2, bits - 1})


@pytest.fixture(scope="module")
def family_b(edges):
    """bits -> [(s, n, prime?)]: the full s list at 256 and 512 bits, three values each from the fixture above."""
    out = {}
    for bits in WIDTHS:
        rows = []
        if bits <= 512:
            for s in _s_list(bits):
                for prime in (True, False):
                    n = G.proth(bits, s, 8000 + bits + s, prime)
                    if n is not None:
                        rows.append((s, n, prime))
            n = G.one_without_minus_one(bits, 30, 8500 + bits, tuple(_bases()))[0]
            rows.append((G.trailing_zeros(n - 1), n, False))
        else:
            rows = [(r["s"], r["n"], r["prime"]) for r in _recs(edges, "B", bits)]
        out[bits] = rows
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_b_candidates_have_their_s_and_run_the_tail(bits, family_b):
    rows = list(family_b[bits])
    lane = LIMB * LW[bits]
    want_s = set(_s_list(bits)) if bits <= 512 else {28, lane, bits // 2}
    if bits <= 512:
        # the last one's tail squares 1: some bases give a square root of 1 other than +-1, and the host says "never"
        s, n, _ = rows.pop()
        exits = [G.strong_exit(n, a) for a in _bases()]
        roots = [a for a in _bases() if pow(a, n >> s, n) not in (1, n - 1) and pow(a, (n >> s) * 2, n) == 1]
        assert s >= 31 and len(roots) >= 2 and all(exits[_bases().index(a)] == (False, "never", s - 1) for a in roots)
        assert any(ok for ok, _, _ in exits) and not _prime_to_both(n)
    assert {s for s, _, _ in rows} == want_s
    for s, n, prime in rows:
        assert n.bit_length() == bits and G.trailing_zeros(n - 1) == s
    primes = _assert_primes_agree([n for _, n, _ in rows])
    assert set(primes) == {n for _, n, prime in rows if prime}
    assert {s for s, _, prime in rows if prime} == {s for s in want_s if s <= bits // 2}
    assert {s for s, _, prime in rows if not prime} == want_s
    # a prime's bases that are no residues reach n - 1 only at the last squaring of the tail
    for s, n, prime in rows:
        if prime:
            depth = max(d for ok, how, d in (G.strong_exit(n, a) for a in _bases()[:8]) if how == "squared")
            assert depth >= s - 2, (s, depth)
    # a composite answers "never" only after the whole tail
    deep = [(s, n) for s, n, prime in rows if not prime and s >= bits // 2]
    assert any(G.strong_exit(n, 3) == (False, "never", s - 1) for s, n in deep)


@pytest.mark.parametrize("bits", WIDTHS)
def test_b_verdicts_equal_host(bits, family_b):
    cands = [n for _, n, _ in family_b[bits]]
    bases = _bases()
    assert bits < 2048 or len(cands) * len(bases) <= 300
    _assert_matrix(_device_matrix(cands, bits, bases), _host_matrix(cands, bases), cands, bases, f"B {bits}")


@lru_cache(maxsize=None)
def _d_semiprime(bits, t):
    return G.liar_semiprime(bits, t, 9000 + bits + t)[0]


def _mixed_wave(bits):
    """s = 1 and s >= 100 in turn, prime and composite, with three bases: every wave of four rows holds both depths."""
    shallow_p, shallow_c = _built_prime(bits, 3, 4, 40 + bits), _d_semiprime(bits, 1)
    deep_p, deep_c = G.proth(bits, bits // 2, 8000 + bits + bits // 2, True), (1 << (bits - 1)) + 1
    liar = next(a for a in range(2, 4096) if _strong_test(shallow_c, a)[0])
    return [shallow_p, deep_p, shallow_c, deep_c], [3, liar, 5]


@pytest.mark.parametrize("bits", [256, 512])
def test_b_mixed_depths_in_one_wave(bits):
    cands, bases = _mixed_wave(bits)
    s = [G.trailing_zeros(n - 1) for n in cands]
    assert s == [1, bits // 2, 1, bits - 1] and bits // 2 >= 100
    for wave in range(len(cands) * len(bases) // 4):
        depths = {s[w // len(bases)] for w in range(4 * wave, 4 * wave + 4)}
        assert 1 in depths and max(depths) >= 100
    want = _host_matrix(cands, bases)
    assert want[0].all() and want[1].all() and want[2].any() and not want[2].all() and not want[3].any()
    _assert_matrix(_device_matrix(cands, bits, bases), want, cands, bases, f"B mixed {bits}")


# ---------------------------------------------------------------- C: bases
def _c_bases():
    rng = random.Random(3100)
    rnd = [rng.getrandbits(32) | 1 << 31 if i % 2 else rng.getrandbits(32) for i in range(7)]
    return [2, (1 << 32) - 1, 1, 1 << 31, 0, (1 << 31) + 1, 4, 1 << 16] + rnd


@pytest.fixture(scope="module")
def family_c(edges, family_b):
    p1k = next(n for s, n, prime in family_b[1024] if prime and s == 28)
    c1k = next(r["n"] for r in _recs(edges, "D", 1024) if r["t"] == 3)
    return {256: [_built_prime(256, 1, 64, 1), _d_semiprime(256, 3)], 1024: [p1k, c1k]}


@pytest.mark.parametrize("bits", [256, 1024])
def test_c_bases_are_mixed(bits, family_c):
    bases, cands = _c_bases(), family_c[bits]
    assert {0, 1, 2, 4, 1 << 16, 1 << 31, (1 << 31) + 1, (1 << 32) - 1} < set(bases) and len(set(bases)) == 15
    assert all(0 <= a < 1 << 32 for a in bases)
    assert _assert_primes_agree(cands) == cands[:1]
    widths = [[bases[w % len(bases)].bit_length() for w in range(4 * k, 4 * k + 4)] for k in range(len(cands) * len(bases) // 4)]
    assert any(min(w) <= 2 and max(w) == 32 for w in widths)
    assert any(min(w) == 0 for w in widths)
    # the composite passes some of these bases and fails others; 0 fails and 1 passes for both
    want = _host_matrix(cands, bases)
    assert want[0].sum() == len(bases) - 1 and 1 < want[1].sum() < len(bases) - 1
    assert not want[:, bases.index(0)].any() and want[:, bases.index(1)].all()


@pytest.mark.parametrize("bits", [256, 1024])
def test_c_verdicts_equal_host(bits, family_c):
    bases, cands = _c_bases(), family_c[bits]
    _assert_matrix(_device_matrix(cands, bits, bases), _host_matrix(cands, bases), cands, bases, f"C {bits}")


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("bits", [256, 1024])
def test_c_one_base_throughout(bits, base, family_c):
    cands, bases = family_c[bits], [base] * 5
    want = _host_matrix(cands, bases)
    assert want.all() if base else not want.any()
    _assert_matrix(_device_matrix(cands, bits, bases), want, cands, bases, f"C {bits} base {base}")


# ---------------------------------------------------------------- D: strong liars
@lru_cache(maxsize=None)
def _d_built(bits, t):
    """(n, bases, host results): every liar below 2^12 and the first four from 2^31 on, as many non-liars, ascending."""
    n = _d_semiprime(bits, t)
    low = {a: _strong_test(n, a) for a in range(1 << 12)}
    high, a = {}, 1 << 31
    while sum(v for v, _ in high.values()) < 4 or sum(not v for v, _ in high.values()) < 4:
        high[a] = _strong_test(n, a)
        a += 1
    res = {**low, **high}
    liars = [a for a in low if low[a][0]] + [a for a in high if high[a][0]][:4]
    others = [a for a in low if not low[a][0]][:len(liars) - 4] + [a for a in high if not high[a][0]][:4]
    bases = sorted(liars + others)
    return n, bases, [res[a] for a in bases]


def _d_fixture(rec):
    n = rec["n"]
    liars = [a for a, _ in rec["liars"]]
    span = list(range(rec["scanned_below"])) + list(range(1 << 31, rec["scanned_high_to"] + 1))
    others = [a for a in span if a not in set(liars)]
    low = sum(a < 1 << 31 for a in liars)
    bases = sorted(liars + [a for a in others if a < 1 << 31][:low] + [a for a in others if a >= 1 << 31][:len(liars) - low])
    return n, bases, [_strong_test(n, a) for a in bases]


@pytest.fixture(scope="module")
def family_d(edges):
    out = {(bits, t): _d_built(bits, t) for bits in (256, 512) for t in (1, 3)}
    for bits in (1024, 2048):
        for rec in _recs(edges, "D", bits):
            out[(bits, rec["t"])] = _d_fixture(rec)
    return out


D_CASES = [(bits, t) for bits in WIDTHS for t in (1, 3)]


def test_d_composites_pass_by_every_exit(family_d, edges):
    assert sorted(family_d) == sorted(D_CASES)
    seen = set()
    for (bits, t), (n, bases, res) in family_d.items():
        assert n.bit_length() == bits and G.trailing_zeros(n - 1) == t
        assert _assert_primes_agree([n]) == []
        exits = {how for ok, how in res if ok}
        assert exits == {"one", "minus_one"} if t == 1 else "squared" in exits and exits <= PASSING, (bits, t, exits)
        seen |= exits
        nl = sum(ok for ok, _ in res)
        assert 2 * nl - 4 <= len(bases) <= 2 * nl and len(set(bases)) == len(bases)
        assert nl >= ((900 if t == 1 else 500) if bits <= 512 else 8) and max(bases) >= 1 << 31
        assert bits < 2048 or len(bases) <= 150
    assert seen == PASSING
    for rec in (r for r in edges if r["family"] == "D"):        # the fixture's liars are the host's, exits included
        n, bases, res = family_d[(rec["bits"], rec["t"])]
        assert [[a, how] for a, (ok, how) in zip(bases, res) if ok] == rec["liars"]


@pytest.mark.parametrize("bits,t", D_CASES)
def test_d_verdicts_equal_host(bits, t, family_d):
    n, bases, res = family_d[(bits, t)]
    want = np.array([[ok for ok, _ in res]], dtype=np.uint8)
    _assert_matrix(_device_matrix([n], bits, bases), want, [n], bases, f"D {bits} t={t}")


# ---------------------------------------------------------------- E: the carry of x + offset
def _e_lengths(bits):
    lane = LIMB * LW[bits]
    return sorted({28, 56, lane, 2 * lane, bits - 2})


def _ones_below(bits, L, rng):
    hb = bits - L
    hi = rng.getrandbits(hb) | 1 << (hb - 1)
    if hi == (1 << hb) - 1:
        hi -= 1                                                 # not 2^bits - 1: nothing above it has `bits` bits
    return hi << L | (1 << L) - 1


@pytest.fixture(scope="module")
def family_e(family_b):
    """bits -> ([(L, start)], host's primes): the low L bits all ones under a random high part, then (L = None) low bits
    all zero, then a prime. At 2048 bits, where one host search takes seconds, L = one lane and L = BITS / 2 are the
    fixture's Proth primes less 2 (the prime is the first number the search meets), L = BITS - 2 as elsewhere, no more."""
    from flex.crypto.paillier import _bigint
    out = {}
    for bits in WIDTHS:
        rng = random.Random(5000 + bits)
        lane = LIMB * LW[bits]
        if bits == 2048:
            starts = [(s, n - 2) for s, n, prime in family_b[bits] if prime and s in (lane, bits // 2)]
            starts.append((bits - 2, _ones_below(bits, bits - 2, rng)))
        else:
            starts = [(L, _ones_below(bits, L, rng)) for L in _e_lengths(bits)]
            starts.append((None, (rng.getrandbits(bits - 2 * lane) | 1 << (bits - 2 * lane - 1)) << 2 * lane))
            starts.append((None, _bigint.next_prime(_seeded_start(bits, 5100 + bits))))
        out[bits] = starts, [_bigint.next_prime(x) for _, x in starts]
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_e_starts_carry_out_of_their_ones(bits, family_e):
    starts, want = family_e[bits]
    lane = LIMB * LW[bits]
    ones = [(L, x) for L, x in starts if L is not None]
    assert [L for L, _ in ones] == (_e_lengths(bits) if bits < 2048 else [lane, bits // 2, bits - 2])
    for L, x in ones:
        assert x.bit_length() == bits and x & ((1 << L) - 1) == (1 << L) - 1
        assert (x + 2) >> L == (x >> L) + 1 and (x + 2).bit_length() == bits      # x + 2 carries out of bit L
    if bits < 2048:
        zero, prime = starts[-2][1], starts[-1][1]
        assert zero % 2 == 0 and zero & ((1 << 2 * lane) - 1) == 0 and zero.bit_length() == bits
        assert _assert_primes_agree([prime]) == [prime] and prime.bit_length() == bits
    assert _assert_primes_agree(want) == want
    assert all(0 < w - x < 4 * bits for w, (_, x) in zip(want, starts))           # each within the default window


@pytest.mark.parametrize("bits", WIDTHS)
def test_e_search_equals_host(bits, family_e):
    starts, want = [x for _, x in family_e[bits][0]], family_e[bits][1]
    primes, passes = _device_search(starts, bits)
    _assert_search(primes, want, starts, f"E {bits}")
    assert passes == [1] * len(starts), passes


# ---------------------------------------------------------------- F: pass 2 rejects; the window refills
@lru_cache(maxsize=None)
def _f_composite(bits, long_gap):
    """A family-D composite that passes base 3 -- with long_gap, the next prime more than 64 above n - 2."""
    return G.base3_pseudoprime(bits, long_gap, 9500 + bits)


@pytest.mark.parametrize("long_gap", [False, True])
@pytest.mark.parametrize("bits", [256, 512])
def test_f_composite_passes_base_3_only(bits, long_gap):
    from flex.crypto.paillier import _bigint
    n = _f_composite(bits, long_gap)
    x = n - 2
    assert n.bit_length() == bits == x.bit_length() and G.no_small_factor(n)
    assert _strong_test(n, 3)[0] and _bigint._SMALL_PRIMES[0] == 3
    assert not all(_strong_test(n, a)[0] for a in _bases()[1:])
    assert _assert_primes_agree([n]) == []
    want = _bigint.next_prime(x)
    assert want > n and (not long_gap or want - x > 64)
    assert want - x < 4 * bits                                  # one default window holds the answer


@pytest.mark.parametrize("bits", [256, 512])
def test_f_pass_2_rejects_and_moves_on(bits):
    from flex.crypto.paillier import _bigint, _native
    n = _f_composite(bits, False)
    primes, passes = _device_search([n - 2], bits)
    launches = _native.prime_last_times()[3]
    _assert_search(primes, [_bigint.next_prime(n - 2)], [n - 2], f"F(i) {bits}")
    assert passes == [1] and launches >= 2, (passes, launches)


@pytest.mark.parametrize("bits", [256, 512])
def test_f_window_refills_after_its_only_survivor(bits):
    from flex.crypto.paillier import _bigint
    n = _f_composite(bits, True)
    primes, passes = _device_search([n - 2], bits, window=64)
    _assert_search(primes, [_bigint.next_prime(n - 2)], [n - 2], f"F(ii) {bits}")
    assert passes[0] >= 2 and passes[0] == -(-(primes[0] - (n - 2)) // 64), passes


# ---------------------------------------------------------------- G: one batch, starts at different stages
@lru_cache(maxsize=None)
def _g_starts():
    from flex.crypto.paillier import _bigint
    quick = next(x for x in (_seeded_start(512, 6000 + k) for k in range(200)) if _bigint.next_prime(x) - x <= 64)
    return (quick, _seeded_start(512, 5), _f_composite(512, False) - 2, (1 << 512) - 33, quick)


def test_g_starts_are_at_different_stages():
    from flex.crypto.paillier import _bigint
    quick, slow, liar, over, again = _g_starts()
    assert again == quick and _bigint.next_prime(quick) - quick <= 64
    assert _bigint.next_prime(slow) - slow == 400
    assert _strong_test(liar + 2, 3)[0] and not _bigint.is_probable_prime(liar + 2)
    assert over.bit_length() == 512 and over + 64 >= 1 << 512


def test_g_batch_equals_single_calls_and_host():
    from flex.crypto.paillier import _bigint
    starts = list(_g_starts())
    primes, passes = _device_search(starts, 512, window=64)
    assert primes[3] is None and passes[3] == -1
    live = [0, 1, 2, 4]
    _assert_search([primes[i] for i in live], [_bigint.next_prime(starts[i]) for i in live], [starts[i] for i in live], "G")
    singles = [_device_search([starts[i]], 512, window=64) for i in live]
    assert [primes[i] for i in live] == [s[0][0] for s in singles]
    assert [passes[i] for i in live] == [s[1][0] for s in singles]
    assert passes[0] == 1 and passes[1] == 7 and passes[2] >= 1 and passes[4] == 1


# ---------------------------------------------------------------- H: more than 2^22 work items
def test_h_second_trip_of_the_grid_stride_loop(family_a):
    cands_a = [n for _, n in family_a[256]]
    five = [cands_a[1], _d_semiprime(256, 1), cands_a[2], _d_semiprime(256, 3), cands_a[8]]
    bases64 = _bases() + _c_bases() + [a for a in range(6, 24) if a not in _bases()][:9]
    assert len(set(bases64)) == 64 and len(_assert_primes_agree(five)) == 3
    tile = _host_matrix(five, bases64)
    assert all(0 < tile[i].sum() < 64 for i in (1, 3))            # the composites pass some bases
    ncand, nbases = 1025, 4096
    assert ncand * nbases > 4 << 20                              # the grid is capped at 2^20 blocks of four rows
    cands = [five[i % 5] for i in range(ncand)]
    bases = [bases64[j % 64] for j in range(nbases)]
    want = np.tile(tile, (ncand // 5, nbases // 64))
    assert want.shape == (ncand, nbases)
    _assert_matrix(_device_matrix(cands, 256, bases), want, cands, bases, "H")


# ---------------------------------------------------------------- I: next_primes' host fallback
def test_i_next_primes_hands_one_start_to_the_host(monkeypatch):
    from flex.crypto.paillier import _bigint, _native
    monkeypatch.delenv("FLEXPAI_KEYGEN_GPU", raising=False)
    assert _bigint.keygen_on_device(256)
    starts = [(1 << 256) - 3, _seeded_start(256, 61)]
    want = [_bigint.next_prime(x) for x in starts]
    assert want[0].bit_length() == 257 and want[1].bit_length() == 256
    before = _native.prime_stats()
    got = _bigint.next_primes(starts, 256)
    after = _native.prime_stats()
    _assert_search(got, want, starts, "I")
    assert after["host_fallbacks"] == before["host_fallbacks"] + 1
    assert after["device_searches"] == before["device_searches"] + 1
