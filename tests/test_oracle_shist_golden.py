"""The oracle against the reference-generated vectors of the sparse histogram (tests/golden/make_golden_shist.py): cells off
the default bin are add_k over the stored members, default cells T - S by add_k, mul_scalar(-1) and add_k."""
import json
import math
import os

import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gshist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_shist.json")) as f:
        return json.load(f)


def oracle_cells(g, cs, es, key):
    """[(ciphertext, exponent) or None] and counts per cell (v, f, b), by the contract of pai_histogram_sparse."""
    N, F, B, nodes = g["N"], g["F"], g["B"], g["nodes"]
    ip, ix, dt = g["indptr"], g["indices"], g["data"]
    stored = [{ix[t]: dt[t] for t in range(ip[i], ip[i + 1])} for i in range(N)]
    fold = lambda mem: O.add_k([cs[i] for i in mem], [es[i] for i in mem], key)
    cells, counts = [], []
    for v in range(nodes):
        members = [i for i in range(N) if g["node"][i] == v]
        for f in range(F):
            z = g["default_bin"][f]
            for b in range(B):
                if b != z:
                    mem = [i for i in members if stored[i].get(f) == b]
                    counts.append(len(mem))
                    cells.append(fold(mem) if mem else None)
                    continue
                rest = [i for i in members if f in stored[i] and stored[i][f] != z]
                counts.append(len(members) - len(rest))
                if len(members) == len(rest):
                    cells.append(None)
                    continue
                T, ET = fold(members)
                if rest:
                    S, ES = fold(rest)
                    neg, en = O.mul_scalar(S, ES, -1, key)
                    T, ET = O.add_k([T, neg], [ET, en], key)
                cells.append((T, ET))
    return cells, counts


@pytest.mark.parametrize("nb", ["1024", "2048"])
def test_oracle_reproduces_the_sparse_histogram_fixture(golden, gshist, nb):
    k = golden["keys"][nb]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    case = gshist["cases"][nb]
    cs, es = [int(h, 16) for h in case["c"]], case["e"]
    assert len(set(es)) > 3                                     # exponents differ inside the cells
    cells, counts = oracle_cells(gshist, cs, es, key)
    assert counts == case["counts"]
    want = [None if c is None else (int(c[0], 16), c[1]) for c in case["cells"]]
    assert cells == want
    # the cases the fixture has to hold: an empty default cell, a default cell that is T itself, a feature without one
    F, B = gshist["F"], gshist["B"]
    at = lambda v, f, b: (v * F + f) * B + b
    v5 = gshist["node"][5]                                     # the sample with the empty row: feature 2's only default entry
    assert want[at(1 - v5, 2, 1)] is None and counts[at(1 - v5, 2, 1)] == 0 and counts[at(v5, 2, 1)] == 1
    members = [i for i in range(gshist["N"]) if gshist["node"][i] == 0]
    assert want[at(0, 3, 0)] == O.add_k([cs[i] for i in members], [es[i] for i in members], key)
    ip, ix, dt = gshist["indptr"], gshist["indices"], gshist["data"]
    assert gshist["default_bin"][1] >= B and B in dt and ip[5] == ip[6] and -1 in gshist["node"]
    # a default cell decrypts to the plain sum over the samples whose entry is at the default bin, stored or not: the
    # subtraction is exact on the encodings, so only decode's two roundings (int to float, times 16^-e) separate them
    vals = [float.fromhex(h) for h in case["x"]]
    for v, f in ((0, 0), (1, 0), (0, 4), (1, 4)):
        z = gshist["default_bin"][f]
        row = lambda i: {ix[t]: dt[t] for t in range(ip[i], ip[i + 1])}
        mem = [i for i in range(gshist["N"]) if gshist["node"][i] == v and row(i).get(f, z) == z]
        c, e = want[at(v, f, z)]
        got = O.decrypt_value(c, e, key)
        assert abs(got - math.fsum(vals[i] for i in mem)) <= 4 * 2.0 ** -53 * math.fsum(abs(vals[i]) for i in mem)
