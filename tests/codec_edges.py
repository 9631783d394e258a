"""Case lists and expected results for the fixed-point codec at its edges (a helper module, not a test): the decode of a
decrypted plaintext (decode_element in csrc/kernels.hpp, decode_lane in csrc/kernels_dec.hpp) and the encoders of
csrc/device_ops.hpp. Everything is built from Python integers and oracle/paillier_oracle.py; test_codec_edges_cpu.py
validates the lists against independent integer models, test_gpu_codec_edges.py runs them on the kernels.

Decode. A case is (name, class, plaintext residue x, exponent e, signed mantissa M). The kernels take |M| from 28-bit
limbs, keep its top 64 bits and one sticky bit for the rest, round half-even to 53 bits and scale by 16^-e. The "kept
part" of a B-bit mantissa is its top 53 bits, the "half bit" is bit B - 54, the 64-bit window starts at bit B - 64.
Exponents beyond +-300 are never given to the oracle (16^(2^29) is a 2^31-bit integer); the rule it follows is written
out in expect_decode:
  e >= 269              16.0^-e is 0.0, so the value is +-0.0 with the mantissa's sign (float(M) is taken first: a
                        mantissa of 2^1024 - 2^970 or more is still "int too large to convert to float")
  e <= -16, M != 0      M 16^-e has 65 bits or more: PAI_EL_INT_BIG
  M == 0                0.0 for e > 0, the int 0 otherwise

Encode. PAI_EXP_AUTO follows oracle.encode. PAI_EXP_FIXED at exponent fexp is round-half-even(v 16^fexp) on the exact
rational value (for an int and fexp < 0: of float(v), which the reference forms first), the reference's |v| < 1e-200 -> 0
cut before it; where |m| >= 2^63 the 64-bit encoder answers PAI_EL_ENC_RANGE, as do NaN and +-inf."""
import math
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle import paillier_oracle as O

EL_OK, EL_INT, EL_INT_BIG, EL_OVERFLOW, EL_FLOAT_OVF, EL_ENC_RANGE = 0, 1, 2, 3, 4, 5     # include/flexpai.h PAI_EL_*
LB = 28                                                                                  # bits of a limb
BITLENS = (1, 28, 29, 52, 53, 54, 55, 56, 57, 63, 64, 65, 66, 84, 85, 92, 93, 112, 113, 1023, 1024)
BITLENS_WIDE = (1025, 1036, 1037)                   # where max_int allows, and bits(max_int)
E_POS = (1, 2, 13, 255, 256, 262, 268, 269, 300, 2 ** 29 - 1, 2 ** 29, 2 ** 30, 2 ** 31 - 1)
E_NONPOS = (0, -1, -2, -15, -16, -255, -2 ** 29, -2 ** 31)
E_CYCLE = E_POS[1:] + E_NONPOS                      # every mantissa meets e = 1 and two of these
ORACLE_E = 300                                      # |e| up to which oracle.decode is asked
DBL_TOP = (1 << 1024) - (1 << 970)                  # the first integer that does not convert to a float
DOUBLE_RANGE = (("largest-double", (1 << 1024) - (1 << 971)), ("below-tie", DBL_TOP - 1), ("tie-to-2^1024", DBL_TOP),
                ("2^1024-1", (1 << 1024) - 1), ("2^1024", 1 << 1024))
KEPT = (1 << 52) + 0x5A5A5A5A5A5A4                  # an even 53-bit kept part; KEPT + 1 is the odd one

Case = namedtuple("Case", "name cls x e M")
Want = namedtuple("Want", "st bits mant")           # bits: the float64 pattern of val (None: not pinned); mant for EL_INT


def f64_bits(v) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def patterns(B):
    """[(pattern name, B-bit mantissa)]: the rounding patterns the length allows. Below 54 bits nothing is dropped."""
    out = [("pow2", 1 << (B - 1)), ("ones", (1 << B) - 1)]
    if B < 54:
        return out[:1] if B == 1 else out
    drop = B - 53
    h = drop - 1                                    # position of the half bit
    for par, nm in ((0, "even"), (1, "odd")):
        tie = (KEPT + par) << drop | 1 << h
        out.append((f"tie-{nm}", tie))
        for bit, what in ((0, "bit0"), (27, "bit27"), (28, "bit28"), (h - 1, "below-half")):
            if 0 <= bit < h:
                out.append((f"tie-{nm}+{what}", tie | 1 << bit))
        if h > 0:
            out.append((f"under-half-{nm}", (KEPT + par) << drop | ((1 << h) - 1)))
        if B > 64 and (B - 64) % LB:                # the limb that holds bit B - 64 also holds bits below the window
            k = (B - 64) // LB
            out.append((f"tie-{nm}+straddle-top", tie | 1 << (B - 65)))
            out.append((f"tie-{nm}+straddle-low", tie | 1 << (k * LB)))
    return out


PATTERN_CLASSES = sorted({nm for B in (113, 1024) for nm, _ in patterns(B)})


def decode_cases(key):
    """The decode cases of one key, mantissas above max_int left out."""
    n, mx = key.n, key.max_int
    cases, cyc = [], 0

    def add(name, cls, M, e):
        if abs(M) <= mx:
            cases.append(Case(f"{name}:e={e}", cls, M % n, e, M))

    lens = list(BITLENS) + [b for b in BITLENS_WIDE + (mx.bit_length(),) if b <= mx.bit_length() and b not in BITLENS]
    for B in lens:
        for nm, mag in patterns(B):
            for M in (mag, -mag):
                for e in (1, E_CYCLE[cyc % len(E_CYCLE)], E_CYCLE[(cyc + 9) % len(E_CYCLE)]):
                    add(f"B{B}:{nm}:{'-' if M < 0 else '+'}", (f"B{B}", nm), M, e)
                cyc += 1
    for nm, mag in DOUBLE_RANGE:
        for M in (mag, -mag):
            for e in (1, 13, 268, 269, 2 ** 30, 0, -1, -2 ** 31):
                add(f"double-range:{nm}:{'-' if M < 0 else '+'}", ("double-range", nm), M, e)
    for B, e in ((63, 0), (59, -1), (55, -2), (3, -15), (64, 0), (60, -1), (56, -2), (4, -15)):     # B + 4|e| = 63, 64
        for mag in ((1 << B) - 1, 1 << (B - 1), (1 << (B - 1)) + 1):
            for M in (mag, -mag):
                add(f"int-seam:B{B}:{M:+#x}", ("int-seam", B - 4 * e), M, e)
    add("int-seam:-2^63", ("int-seam", "-2^63"), -(1 << 63), 0)
    add("int-seam:+2^63", ("int-seam", "+2^63"), 1 << 63, 0)
    for e in (300, 1, 2 ** 30, 2 ** 31 - 1, 0, -16, -2 ** 29, -2 ** 31):
        add("zero", ("zero", e > 0), 0, e)
    # the sign band: residues, not mantissas (max_int + 1 .. n - max_int - 1 is the overflow band)
    for nm, x in (("max_int", mx), ("max_int+1", mx + 1), ("n-max_int-1", n - mx - 1), ("n-max_int", n - mx), ("n-1", n - 1)):
        M = x if x <= mx else x - n if x >= n - mx else None
        for e in (1, 2, 300, 2 ** 30, 0, -1, -2 ** 31):
            cases.append(Case(f"sign-band:{nm}:e={e}", ("sign-band", nm), x, e, M))
    return cases


def expect_decode(x, e, n, max_int) -> Want:
    """What pai_decrypt must report for the plaintext residue x at exponent e."""
    if abs(e) <= ORACLE_E:
        try:
            want = O.decode(x, e, n, max_int)
        except OverflowError as err:
            return Want(EL_OVERFLOW if "Overflow detected in decode number" in str(err) else EL_FLOAT_OVF, None, None)
        if isinstance(want, float):
            return Want(EL_OK, f64_bits(want), None)
        if abs(want) < 1 << 63:                     # "fits int64" as the kernels read it: 63 bits, so not -2^63
            return Want(EL_INT, f64_bits(float(want)), want)
        return Want(EL_INT_BIG, None, None)
    if max_int < x < n - max_int:
        return Want(EL_OVERFLOW, None, None)
    M = x if x <= max_int else x - n
    if e > 0:
        if abs(M) >= DBL_TOP:
            return Want(EL_FLOAT_OVF, None, None)
        return Want(EL_OK, f64_bits(-0.0 if M < 0 else 0.0), None)
    return Want(EL_INT, f64_bits(0.0), 0) if M == 0 else Want(EL_INT_BIG, None, None)


# --------------------------------------------------------------------------- encode
AUTO_FE = tuple(range(-663, -654)) + tuple(range(-3, 61)) + tuple(range(1017, 1025))
FIXED_EXPS = (-16, -5, -1, 0, 1, 5, 13, 15, 16, 64, 255, 256, 300)
_NONFINITE = (float("nan"), float("inf"), float("-inf"))


def f64_auto_values():
    """+-(2^52 + t) 2^(fe - 53), t in 0..15: frexp exponent fe, so 53 - fe runs over all four residues mod 4 on both
    sides of zero, with up to three bits dropped and their ties; then the specials."""
    v = [s * math.ldexp((1 << 52) + t, fe - 53) for fe in AUTO_FE for t in range(16) for s in (1, -1)]
    v += [1e-200, np.nextafter(1e-200, 0.0), np.nextafter(1e-200, 1.0), 5e-324, 2.2250738585072014e-308,
          1.7976931348623157e308, -1.7976931348623157e308, 0.0, -0.0, *_NONFINITE]
    return np.array(v, dtype=np.float64)


def f32_values():
    return np.array([1e-45, -1e-45, 1.1754944e-38, 3.4028235e38, -3.4028235e38, 1.0 / 3.0, -1.0 / 3.0, 0.0, -0.0, 1.0, -1.5,
                     *_NONFINITE], dtype=np.float32)


def i64_auto_values():
    return np.array([0, 1, -1, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 63 - 1, -(2 ** 63) + 1, -(2 ** 63)], dtype=np.int64)


def f64_fixed_values():
    """The floats of the fixed-exponent runs: ties at fexp = 0 and 1, both sides of the 1e-200 cut, the double whose
    mantissa at fexp = 0 is the largest below 2^63, the largest double, and the non-finite ones."""
    return np.array([0.0, -0.0, 1.0, -1.5, 0.1, 1.0 / 3.0, 2.0 ** 51 + 0.5, -(2.0 ** 51 + 1.5), 0.03125, 0.09375, -123456.789,
                     1e10, 1e-200, np.nextafter(1e-200, 0.0), 5e-324, float((2 ** 53 - 1) << 10), 2.0 ** 63,
                     1.7976931348623157e308, *_NONFINITE], dtype=np.float64)


def i64_fixed_values(fexp):
    v = [0, 1, -1, 2 ** 59 - 1, -(2 ** 59 - 1), 2 ** 59, -(2 ** 59)]
    if fexp < 0:                                    # 54 bits or more: int -> double rounds before the scaling
        v += [2 ** 54 + 1, -(2 ** 54 + 3), 2 ** 62 + 2 ** 8 + 1, 2 ** 63 - 1, -(2 ** 63) + 1, (2 ** 53 + 1) << 4]
    return np.array(v, dtype=np.int64)


def _py(v):
    return int(v) if isinstance(v, (int, np.integer)) else v if isinstance(v, np.float32) else float(v)


def expect_encode_auto(v, key):
    """(status, signed mantissa, exponent) under PAI_EXP_AUTO, from oracle.encode."""
    v = _py(v)
    if not isinstance(v, int) and not math.isfinite(float(v)):
        return EL_ENC_RANGE, None, None
    m, e = O.encode(v, key.n, key.max_int)
    return EL_OK, m if m <= key.max_int else m - key.n, e


def fixed_model(v, fexp):
    """The exact integer round-half-even(v 16^fexp) (None: not finite) with the reference's cut and int -> float step."""
    v = _py(v)
    if not isinstance(v, int) and not math.isfinite(float(v)):
        return None
    if abs(float(v)) < 1e-200:
        return 0
    if isinstance(v, int) and fexp >= 0:
        return v * 16 ** fexp
    return round(Fraction(float(v)) * Fraction(16) ** fexp)          # Fraction.__round__ rounds half to even


def expect_encode_fixed(v, fexp):
    m = fixed_model(v, fexp)
    if m is None or abs(m) >= 1 << 63:
        return EL_ENC_RANGE, None, None
    return EL_OK, m, fexp


def c0(m, key):
    """The unobfuscated ciphertext of the signed mantissa m (oracle.raw_encrypt with r = 1)."""
    return (1 + key.n * (m % key.n)) % key.nsquare
