#!/usr/bin/env python3
"""The fused encrypted-by-plain matrix product (ibond-flex_amd/csrc/kernels_mm.hpp: k_mm_sign, k_mm_tab, k_mm_acc):

  * counts(): Montgomery products per chunk of KC operands of one output on the term path (k_mul + batch inversion +
    first k_add level) and on the fused path, for (m, K, d, nw, share of negative rows, KC). Counts, not times.
  * fused_dot(): a big-int model of the fused schedule -- the scalar encoding, the 4-bit digits of |M|, the shift of a
    digit by D = E - e whole windows, the sign selecting the table of c or of c^-1, zero terms (value 1, but their
    exponent counts towards E), padding of a last short chunk, and the k_add reduction of the chunk partials -- that
    tests/test_mm_model.py checks against the oracle's mul_scalar + add_k.

    python tools/mm_model.py [--m 1] [--K 4096] [--d 64] [--nw 14] [--neg 1.0] [--kc 16]"""
import argparse
import json
import math
from fractions import Fraction

KC = 16          # MM_KC: operands per k_mm_acc instance


# --------------------------------------------------------------------------- scalar encoding (precision None)
def encode(s):
    """(M, e): the signed mantissa and the exponent of FixedPointNumber.encode for an int or a float scalar
    (fixedpoint_number.py:46-90: ints keep exponent 0, floats get e = floor((53 - frexp(v).exp) / 4) and
    M = round_half_even(v 16^e) on the exact value; |v| < 1e-200 is the int 0). float32 values widen exactly."""
    if hasattr(s, "dtype") and s.dtype.kind == "i" or isinstance(s, int):
        return int(s), 0
    v = float(s)
    if abs(v) < 1e-200:
        return 0, 0
    e = (53 - math.frexp(v)[1]) // 4
    x = Fraction(v) * Fraction(16) ** e
    q, r = divmod(x.numerator, x.denominator)
    if 2 * r > x.denominator or (2 * r == x.denominator and q & 1):
        q += 1
    return q, e


def windows(mag: int) -> int:
    """4-bit windows of |M| as the kernels count them ((67 - clz64) / 4)."""
    return (mag.bit_length() + 3) // 4


# --------------------------------------------------------------------------- the fused schedule
def table(c: int, n2: int):
    """k_mm_tab: c^0 .. c^15 mod n^2 by 14 products after the first."""
    rows = [1, c % n2]
    for _ in range(14):
        rows.append(rows[-1] * rows[1] % n2)
    return rows


def chunk_partial(cts, exps, scalars, n2, stats=None):
    """k_mm_acc for one output and one chunk: (partial, E). cts / exps: the chunk's ciphertexts and exponents,
    scalars: the matching column entries of x. ZeroDivisionError where the reference raises it (a negative scalar on a
    ciphertext without inverse)."""
    ops = []
    for c, ec, s in zip(cts, exps, scalars):
        M, es = encode(s)
        base = pow(c, -1, n2) if M < 0 else c        # pow raises ValueError: mapped below
        ops.append((abs(M), ec + es, table(base, n2)))
    E = max(e for _, e, _ in ops)                    # zero terms count
    top = max([windows(mag) + (E - e) for mag, e, _ in ops if mag] or [0])
    acc, started = 1, False
    for w in range(top - 1, -1, -1):
        if started:
            for _ in range(4):
                acc = acc * acc % n2
                if stats is not None:
                    stats["squarings"] += 1
        for mag, e, tab in ops:
            sh = w - (E - e)
            dig = (mag >> (4 * sh)) & 15 if 0 <= sh < 16 else 0
            if dig:
                acc = acc * tab[dig] % n2
                started = True
                if stats is not None:
                    stats["products"] += 1
    return acc, E


def add_tree(parts, exps, n2):
    """k_add over the chunk partials: prod P^(16^(E - e)), E the maximum (any grouping gives the same residue)."""
    E = max(exps)
    acc = 1
    for p, e in zip(parts, exps):
        acc = acc * pow(p, 16 ** (E - e), n2) % n2
    return acc, E


def fused_dot(cts, exps, col, n2, kc=KC, stats=None):
    """One output of the fused product: sum_k cts[k] (x) col[k] as (ciphertext, exponent)."""
    K = len(cts)
    assert len(exps) == K and len(col) == K and K > 0
    parts, pexps = [], []
    try:
        for k0 in range(0, K, kc):
            p, e = chunk_partial(cts[k0:k0 + kc], exps[k0:k0 + kc], col[k0:k0 + kc], n2, stats)
            parts.append(p)
            pexps.append(e)
    except ValueError as err:                        # pow(c, -1, n2) without inverse
        raise ZeroDivisionError("invert() no inverse exists") from err
    return add_tree(parts, pexps, n2)


def neg_rows(x_rows):
    """k_mm_sign: per row k of x (a sequence of rows), whether some column encodes to M < 0."""
    return [any(encode(s)[0] < 0 for s in row) for row in x_rows]


# --------------------------------------------------------------------------- product counts
INV_PER_VALUE = 6     # k_inv_up: load (to Montgomery) + prefix product; k_inv_down: r, out of the domain, load, I update


def counts(m=1, K=4096, d=64, nw=14, neg=1.0, kc=KC):
    """Montgomery products per output and chunk of kc operands, all scalars at nw windows and equal exponents (D = 0).
    term:  kc x (to Montgomery 1 + table 14 + squarings 4 (nw - 1) + window products nw - 1 + out of the domain 1
           + the batch inversion's INV_PER_VALUE, which runs over every term) + the first k_add level (kc - 1 products
           + 1 correction).
    fused: 4 (nw - 1) squarings + nw kc table products + 1 (out of the domain), plus the chunk's share of the tables:
           kc ciphertexts x (15 products, and 15 + INV_PER_VALUE more on a share `neg` of the rows) spread over d columns.
    m only scales both sides."""
    term = kc * (1 + 14 + 4 * (nw - 1) + (nw - 1) + 1 + INV_PER_VALUE) + kc
    chain = 4 * (nw - 1) + nw * kc + 1
    tables = kc * (15 + neg * (15 + INV_PER_VALUE)) / d
    chunks = -(-K // kc)
    return {"m": m, "K": K, "d": d, "nw": nw, "neg_rows": neg, "kc": kc,
            "term_per_chunk": term, "fused_chain_per_chunk": chain, "fused_tables_per_chunk": round(tables, 2),
            "fused_per_chunk": round(chain + tables, 2), "ratio_term_over_fused": round(term / (chain + tables), 2),
            "term_total": term * chunks * m * d, "fused_total": round((chain + tables) * chunks * m * d),
            "table_rows": int(16 * m * K * (1 + neg))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--nw", type=int, default=14)
    ap.add_argument("--neg", type=float, default=1.0)
    ap.add_argument("--kc", type=int, default=KC)
    a = ap.parse_args()
    print(json.dumps(counts(a.m, a.K, a.d, a.nw, a.neg, a.kc)))


if __name__ == "__main__":
    main()
