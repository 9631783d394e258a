"""Case lists and expected results for the plain scalar operand of the homomorphic operators at the encoder's edges (a
helper module, not a test): pai_mul, pai_add_plain, pai_matmul and pai_segment_dot, whose kernels (k_mul, k_plain,
k_mm_sign, k_mm_acc, k_sd_sign, k_sd_acc) each do something of their own with the (M, e) the shared encoder returns: the
window count, the negation of M, e entering a maximum, the shifted multiplier of n. Everything is built from Python
integers and oracle/paillier_oracle.py; test_scalar_edges_cpu.py validates the lists, test_gpu_scalar_edges.py runs them
on the kernels and through the package.

What the scalars do (FACTS, checked against the oracle on the CPU):
  2^60 - 1          15 all-ones windows of 4 bits; +-2^60 opens the 16th; +-(2^63 - 1) fills it; INT64_MIN is |M| = 2^63
  +-1e-200          the smallest magnitude that is not cut to the int 0: e = 179, a 52-bit mantissa
  +-nextafter(1e-200, 0), +-5e-324, +-DBL_MIN    the int 0 at exponent 0
  +-DBL_MAX         e = -243, a 53-bit mantissa (the most a float has: 14 windows, so only int64 reaches 16)
  +-1e-45 (f32)     the smallest denormal float32: e = 50;  +-FLT_MAX: e = -19
  nan, +-inf        do not encode: ValueError and OverflowError in the reference

A scalar that does not encode is, on the C ABI, "the factor 1": the term (1, exp_i + 0) with status PAI_EL_ENC_RANGE
(include/flexpai.h at pai_mul, pai_matmul, pai_segment_dot). expect_dot / expect_segdot apply that rule to oracle terms
with factor_one=True and raise the oracle's exception without it."""
import math

import numpy as np

from oracle import paillier_oracle as O

EL_OK, EL_FLOAT_OVF, EL_ENC_RANGE = 0, 4, 5          # include/flexpai.h PAI_EL_*
INT32_MIN = -(1 << 31)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
DBL_MAX, DBL_MIN = 1.7976931348623157e308, 2.2250738585072014e-308
FLT_MAX, FLT_MIN, FLT_DENORM = 3.4028235e38, 1.1754944e-38, 1e-45
CUT = 1e-200                                        # fixedpoint_number.py:56-57: |v| < 1e-200 is the int 0
BELOW_CUT = float(np.nextafter(CUT, 0.0))
NAN, INF = float("nan"), float("inf")


def _pm(*vals):
    return [s * v for v in vals for s in (1, -1)]


I64 = [0, *_pm(1, 15, 16), 2 ** 60 - 1, *_pm(2 ** 60, 2 ** 62), INT64_MAX, -INT64_MAX, INT64_MIN]
F64 = [*_pm(0.0, CUT, BELOW_CUT, 5e-324, DBL_MIN, DBL_MAX, 2.0 - 2.0 ** -52), 0.1, NAN, INF, -INF]
F32 = [*_pm(0.0, FLT_DENORM, FLT_MIN, FLT_MAX), NAN, INF, -INF]
LISTS = {np.int64: I64, np.float64: F64, np.float32: F32}
# the six floats of the 4096-bit runs: a zero, both signs of the cut and of the largest double, one ordinary value
F64_SUBSET = [-0.0, CUT, -CUT, DBL_MAX, -DBL_MAX, 0.1]
# name -> (scalar, dtype, sign of M, bits of |M|, exponent); bits None: not pinned
FACTS = {
    "2^60-1": (2 ** 60 - 1, np.int64, 1, 60, 0), "2^60": (2 ** 60, np.int64, 1, 61, 0), "-2^60": (-2 ** 60, np.int64, -1, 61, 0),
    "int64-max": (INT64_MAX, np.int64, 1, 63, 0), "int64-min": (INT64_MIN, np.int64, -1, 64, 0),
    "cut": (CUT, np.float64, 1, 52, 179), "-cut": (-CUT, np.float64, -1, 52, 179),
    "below-cut": (BELOW_CUT, np.float64, 0, 0, 0), "-below-cut": (-BELOW_CUT, np.float64, 0, 0, 0),
    "denormal": (5e-324, np.float64, 0, 0, 0), "-denormal": (-5e-324, np.float64, 0, 0, 0),
    "dbl-min": (DBL_MIN, np.float64, 0, 0, 0), "-dbl-min": (-DBL_MIN, np.float64, 0, 0, 0),
    "dbl-max": (DBL_MAX, np.float64, 1, 53, -243), "-dbl-max": (-DBL_MAX, np.float64, -1, 53, -243),
    "f32-denormal": (FLT_DENORM, np.float32, 1, None, 50), "-f32-denormal": (-FLT_DENORM, np.float32, -1, None, 50),
    "flt-max": (FLT_MAX, np.float32, 1, None, -19), "-flt-max": (-FLT_MAX, np.float32, -1, None, -19),
}


def scalars(dt, finite_only=False) -> np.ndarray:
    """The whole list of a dtype as an array of it (int64, float64, float32)."""
    v = np.array(LISTS[dt], dtype=dt)
    return v[np.isfinite(v)] if finite_only and dt != np.int64 else v


def py(v, dt):
    """The Python value the reference's operators see for element v of an array of dtype dt."""
    return int(v) if dt == np.int64 else (np.float32(v) if dt == np.float32 else float(v))


def finite(v) -> bool:
    return isinstance(v, (int, np.integer)) or math.isfinite(float(v))


def mantissa(v, key):
    """(signed mantissa, exponent) of the oracle's encoding."""
    m, e = O.encode(v, key.n, key.max_int)
    return (m if m <= key.max_int else m - key.n), e


def windows(M: int) -> int:
    """4-bit windows of |M|."""
    return (abs(M).bit_length() + 3) // 4


def expect_mul(c, e, x, key):
    """(ciphertext, exponent) of c (x) x from the oracle, or the class of the exception it raises."""
    try:
        return O.mul_scalar(c, e, x, key)
    except (ValueError, OverflowError) as err:
        return type(err)


def expect_add(c, e, x, key):
    """(ciphertext, exponent) of c (+) x from the oracle, or the class of the exception it raises."""
    try:
        return O.add_scalar(c, e, x, key)
    except (ValueError, OverflowError) as err:
        return type(err)


def expect_add_status(c, e, x, key):
    """(status, (ciphertext, exponent) or None) of pai_add_plain: a NaN does not encode (PAI_EL_ENC_RANGE), x 16^E of an
    infinity is not a finite double (PAI_EL_FLOAT_OVF), and so is every finite case in which the oracle raises
    OverflowError; its ValueError on a finite scalar (|M| > max_int) is PAI_EL_ENC_RANGE."""
    if not finite(x):
        return (EL_ENC_RANGE if math.isnan(float(x)) else EL_FLOAT_OVF), None
    want = expect_add(c, e, x, key)
    if want is OverflowError:
        return EL_FLOAT_OVF, None
    if want is ValueError:
        return EL_ENC_RANGE, None
    return EL_OK, want


def add_plain_exps(x, dt, key):
    """Ciphertext exponents on which pai_add_plain meets the scalar: both branches of encode_plain_max (E = e0 and
    E > e0) around the scalar's own exponent e0, far below it, and the last exponent before 16^E leaves the doubles.
    A scalar without an exponent of its own takes 13, the e0 of 1.0."""
    if dt == np.int64:
        return [-5, 0, 3]
    e0 = mantissa(x, key)[1] if finite(x) else 13
    return sorted({-300, 0, e0 - 1, e0, e0 + 1, 255})


def term(c, e, x, key, factor_one):
    """One term of a weighted sum. A scalar that does not encode raises the oracle's exception, or is the factor 1 at
    exponent e + 0 where factor_one is set (include/flexpai.h)."""
    want = expect_mul(c, e, x, key)
    if isinstance(want, type):
        if not factor_one:
            raise want(f"the scalar {x!r} does not encode")
        return 1, e + 0
    return want


def _fold(terms, key):
    if not terms:
        return 1, INT32_MIN
    return O.add_k([t[0] for t in terms], [t[1] for t in terms], key)


def expect_dot(cs, es, m, K, x, d, key, factor_one=False):
    """[(ciphertext, exponent)] of the m x d outputs of (m x K ciphertexts) times x (K x d), row-major."""
    dt = x.dtype.type
    return [_fold([term(cs[i * K + k], int(es[i * K + k]), py(x[k, j], dt), key, factor_one) for k in range(K)], key)
            for i in range(m) for j in range(d)]


def expect_segdot(cs, es, idx, off, x, key, factor_one=False):
    """[(ciphertext, exponent)] of the segments; an empty one is (1, INT32_MIN)."""
    dt = x.dtype.type
    return [_fold([term(cs[int(idx[t])], int(es[int(idx[t])]), py(x[t], dt), key, factor_one)
                   for t in range(int(off[s]), int(off[s + 1]))], key) for s in range(len(off) - 1)]
