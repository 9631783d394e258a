"""The codec edge cases of tests/codec_edges.py, validated without a GPU: every expected decode result against an
integer-only model of int -> double rounding, every expected encoding against exact rational rounding, the pattern lists
against what their names say, and the coverage each key keeps after the mantissas above its max_int are dropped."""
import math
from fractions import Fraction

import numpy as np
import pytest

import codec_edges as CE
from oracle import paillier_oracle as O
from test_gpu_key_sizes import _make_key

KEYS = ("K512", "K1024", "K1034T", "K1036", "K2048", "K2071", "K2072", "K4096")
# Classes that need a mantissa above max_int and drop on the keys below 1027 bits; nothing else may drop.
DROPS_BELOW_1027 = {"B1023", "B1024", "B1025", "B1036", "B1037", "double-range"}


@pytest.fixture(scope="module")
def keys(golden):
    return {k: _make_key(k, golden) for k in KEYS}


def model_decode(M, e):
    """(status, bits of val or None, mant or None) of the signed mantissa M at exponent e: kept part, half bit and sticky
    bit from the integer, the double from math.ldexp, times 16.0 ** -e. No oracle, and for e > 0 no int -> float
    conversion of more than 54 bits."""
    a, B = abs(M), abs(M).bit_length()
    if e <= 0:
        if a == 0:
            return CE.EL_INT, CE.f64_bits(0.0), 0
        if B - 4 * e <= 63:
            return CE.EL_INT, CE.f64_bits(math.ldexp(M, -4 * e)), M << (-4 * e)      # at most 63 bits after scaling ...
        return CE.EL_INT_BIG, None, None
    drop = max(B - 53, 0)
    kept = a >> drop
    if drop:
        half = (a >> (drop - 1)) & 1
        sticky = a & ((1 << (drop - 1)) - 1) != 0
        if half and (sticky or kept & 1):
            kept += 1
    try:
        d = math.ldexp(kept, drop)                   # kept has at most 54 bits and is even then: exact
    except OverflowError:
        return CE.EL_FLOAT_OVF, None, None
    return CE.EL_OK, CE.f64_bits((-d if M < 0 else d) * 16.0 ** -e), None


@pytest.mark.parametrize("name", KEYS)
def test_decode_expectations_follow_the_integer_model(keys, name):
    key = keys[name]
    cases = CE.decode_cases(key)
    assert len({(c.x, c.e) for c in cases}) > 1000 or key.n.bit_length() < 1027
    for c in cases:
        want = CE.expect_decode(c.x, c.e, key.n, key.max_int)
        if c.M is None:
            assert want.st == CE.EL_OVERFLOW and key.max_int < c.x < key.n - key.max_int, c.name
            continue
        assert abs(c.M) <= key.max_int and c.M % key.n == c.x, c.name
        got = model_decode(c.M, c.e)
        if got[0] == CE.EL_INT and c.M.bit_length() - 4 * c.e > 53:
            # ... but float(M 16^-e) rounds once there, as ldexp(M) does: the same double
            assert got[1] == CE.f64_bits(float(got[2])), c.name
        assert tuple(want) == got, f"{name} {c.name}: expected {want}, the model gives {got}"


def test_huge_exponent_rule_meets_the_oracle_where_both_apply(keys):
    """The written-out rule for |e| > 300 gives what oracle.decode gives at the exponents both can take."""
    key = keys["K2048"]
    n, mx = key.n, key.max_int
    was = CE.ORACLE_E
    try:
        for x in (0, 1, 5, n - 5, CE.DBL_TOP - 1, n - CE.DBL_TOP + 1, CE.DBL_TOP, n - CE.DBL_TOP, mx, mx + 1, n - mx, n - 1, 1 << 63):
            for e in (269, 270, 300, -16, -17, -300):
                CE.ORACLE_E = 300
                a = CE.expect_decode(x, e, n, mx)
                CE.ORACLE_E = 0
                assert CE.expect_decode(x, e, n, mx) == a, (hex(x), e)
    finally:
        CE.ORACLE_E = was
    assert CE.expect_decode(n - 5, 2 ** 30, n, mx) == CE.Want(CE.EL_OK, CE.f64_bits(-0.0), None)
    assert CE.expect_decode(5, -2 ** 31, n, mx).st == CE.EL_INT_BIG and CE.expect_decode(0, -2 ** 31, n, mx).mant == 0


def test_double_range_and_int_seam_values(keys):
    key = keys["K2048"]
    n, mx = key.n, key.max_int
    top = float.fromhex("0x1.fffffffffffffp+1023")
    want = {"largest-double": CE.EL_OK, "below-tie": CE.EL_OK, "tie-to-2^1024": CE.EL_FLOAT_OVF, "2^1024-1": CE.EL_FLOAT_OVF,
            "2^1024": CE.EL_FLOAT_OVF}
    assert [nm for nm, _ in CE.DOUBLE_RANGE] == list(want)
    for nm, M in CE.DOUBLE_RANGE:
        for s in (1, -1):
            w = CE.expect_decode(s * M % n, 1, n, mx)
            assert w.st == want[nm], nm
            if w.st == CE.EL_OK:
                assert w.bits == CE.f64_bits(s * top / 16.0), nm
            assert CE.expect_decode(s * M % n, 0, n, mx).st == CE.EL_INT_BIG, nm
    assert int(top) == CE.DOUBLE_RANGE[0][1] and CE.DBL_TOP == 2 ** 1024 - 2 ** 970
    for M, st in ((2 ** 63 - 1, CE.EL_INT), (-(2 ** 63) + 1, CE.EL_INT), (-(2 ** 63), CE.EL_INT_BIG), (2 ** 63, CE.EL_INT_BIG)):
        assert CE.expect_decode(M % n, 0, n, mx).st == st, M


def test_patterns_do_what_their_names_say():
    for B in CE.BITLENS + CE.BITLENS_WIDE + (4091,):
        pats = CE.patterns(B)
        names = [nm for nm, _ in pats]
        assert len(set(names)) == len(names)
        for nm, M in pats:
            assert M.bit_length() == B, (B, nm)
            if nm == "pow2":
                assert M == 1 << (B - 1)
            elif nm == "ones":
                assert M + 1 == 1 << B
            if B < 54:
                assert nm in ("pow2", "ones")
                continue
            if nm in ("pow2", "ones"):
                continue
            drop = B - 53
            kept, half, low = M >> drop, (M >> (drop - 1)) & 1, M & ((1 << (drop - 1)) - 1)
            assert kept & 1 == ("odd" in nm), (B, nm)
            if nm.startswith("under-half"):
                assert half == 0 and low == (1 << (drop - 1)) - 1 and low, (B, nm)
                continue
            assert nm.startswith("tie-") and half == 1, (B, nm)
            extra = nm.partition("+")[2]
            if not extra:
                assert low == 0, (B, nm)                       # an exact tie
                continue
            assert low and low & (low - 1) == 0, (B, nm)       # one sticky bit and nothing else
            bit = low.bit_length() - 1
            if extra in ("bit0", "bit27", "bit28"):
                assert bit == int(extra[3:])
                assert (low < 1 << CE.LB) == (extra != "bit28")           # sticky only in limb 0 / only in limb 1
            elif extra == "below-half":
                assert bit == drop - 2
            else:
                k = (B - 64) // CE.LB                          # the limb that straddles the 64-bit window's low end
                assert extra in ("straddle-top", "straddle-low") and B > 64
                assert k * CE.LB <= bit < B - 64 < (k + 1) * CE.LB, (B, nm)
                assert bit == (B - 65 if extra == "straddle-top" else k * CE.LB)
    # the lengths at a limb seam have no straddling limb, their neighbours do
    assert not any("straddle" in nm for nm, _ in CE.patterns(92)) and any("straddle" in nm for nm, _ in CE.patterns(93))
    assert {nm for nm, _ in CE.patterns(1037)} == set(CE.PATTERN_CLASSES)


@pytest.mark.parametrize("name", KEYS)
def test_every_class_keeps_a_case(keys, name):
    key = keys[name]
    nb = key.n.bit_length()
    cases = CE.decode_cases(key)
    kept = {c.cls[0] for c in cases} | {c.cls[1] for c in cases if c.cls[0].startswith("B")}
    need = ({f"B{b}" for b in CE.BITLENS} | set(CE.PATTERN_CLASSES) | {"double-range", "sign-band", "int-seam", "zero"})
    if nb >= 1027:
        assert need <= kept, f"{name} lost {sorted(need - kept)}"
        assert {c.cls[1] for c in cases if c.cls[0] == "double-range"} == {nm for nm, _ in CE.DOUBLE_RANGE}
        assert f"B{key.max_int.bit_length()}" in kept
        if key.max_int >= 1 << 1037:
            assert {"B1025", "B1036", "B1037"} <= kept
    else:
        assert need - kept == DROPS_BELOW_1027 & need, f"{name} lost {sorted(need - kept)}"
    # every pattern meets e = 1 and at least two other exponents; the exponent lists are all used
    by = {}
    for c in cases:
        if c.cls[0].startswith("B"):
            by.setdefault(c.cls[1], set()).add(c.e)
    assert all(1 in es and len(es) >= 3 for es in by.values())
    assert set(CE.E_POS + CE.E_NONPOS) <= {c.e for c in cases}
    assert {("int-seam", 63), ("int-seam", 64), ("int-seam", "-2^63"), ("zero", True), ("zero", False)} <= {c.cls for c in cases}
    assert {c.cls[1] for c in cases if c.cls[0] == "sign-band"} == {"max_int", "max_int+1", "n-max_int-1", "n-max_int", "n-1"}


def test_auto_encodings_follow_the_rational_model(keys):
    key = keys["K1024"]
    vals = [*CE.f64_auto_values(), *CE.f32_values()]
    res = set()
    for v in vals:
        st, m, e = CE.expect_encode_auto(v, key)
        if not math.isfinite(float(v)):
            assert st == CE.EL_ENC_RANGE
            continue
        f = float(v)
        if abs(f) < 1e-200:
            assert (st, m, e) == (CE.EL_OK, 0, 0), v
            continue
        we = (53 - math.frexp(f)[1]) // 4
        assert (st, m, e) == (CE.EL_OK, round(Fraction(f) * Fraction(16) ** we), we), v
        res.add(((53 - math.frexp(f)[1]) % 4, e > 0))
        assert 2 ** 49 <= abs(m) <= 2 ** 53
    assert res == {(r, s) for r in range(4) for s in (False, True)}
    ties = [v for v in CE.f64_auto_values() if math.isfinite(v) and abs(v) >= 1e-200 and
            (Fraction(float(v)) * Fraction(16) ** ((53 - math.frexp(v)[1]) // 4)).denominator == 2]
    assert len(ties) > 100
    for v in CE.i64_auto_values():
        assert CE.expect_encode_auto(v, key) == (CE.EL_OK, int(v), 0)
    assert O.encode(-(2 ** 63), key.n, key.max_int) == (key.n - 2 ** 63, 0)


def test_fixed_encodings_meet_the_oracle_where_a_precision_names_the_exponent(keys):
    key = keys["K2048"]
    checked = 0
    for fexp in CE.FIXED_EXPS:
        prec = 16.0 ** fexp if fexp < 256 else None
        named = prec is not None and math.floor(math.log(prec, 16)) == fexp
        for v in [*CE.f64_fixed_values(), *CE.f32_values(), *CE.i64_fixed_values(fexp)]:
            st, m, e = CE.expect_encode_fixed(v, fexp)
            if st != CE.EL_OK:
                mm = CE.fixed_model(v, fexp)
                assert mm is None or abs(mm) >= 2 ** 63, (v, fexp)
                continue
            assert e == fexp and abs(m) < 2 ** 63
            if named:
                assert O.encode(CE._py(v), key.n, key.max_int, precision=prec) == (m % key.n, fexp), (v, fexp)
                checked += 1
    assert checked > 150
    # both sides of encode_int's +-INT64_MAX bound at fexp = 1, and of the float bound at fexp = 0
    assert CE.expect_encode_fixed(2 ** 59 - 1, 1) == (CE.EL_OK, 2 ** 63 - 16, 1) and CE.expect_encode_fixed(2 ** 59, 1)[0] == CE.EL_ENC_RANGE
    assert CE.expect_encode_fixed(-(2 ** 59), 1)[0] == CE.EL_ENC_RANGE
    assert CE.expect_encode_fixed(float((2 ** 53 - 1) << 10), 0) == (CE.EL_OK, 2 ** 63 - 1024, 0)
    assert CE.expect_encode_fixed(2.0 ** 63, 0)[0] == CE.EL_ENC_RANGE
    assert CE.expect_encode_fixed(np.int64(2 ** 54 + 1), -1) == (CE.EL_OK, 2 ** 50, -1)      # float(v) drops the + 1 first
