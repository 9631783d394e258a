"""The histogram fixture (tests/golden/paillier_golden_hist.json, the reference's own ``+`` chains per cell) against the
CPU oracle: oracle.add_k over each cell's members reproduces every stored (ciphertext, exponent), and the stored counts
follow the cell rule."""
import json
import os

import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ghist():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_hist.json")) as f:
        return json.load(f)


def cell_members(g):
    """Members of every cell in the order (node, feature, bin)."""
    F, B, nodes, bins, node = g["F"], g["B"], g["nodes"], g["bins"], g["node"]
    return [[i for i in range(len(node)) if node[i] == v and bins[i][f] == b]
            for v in range(nodes) for f in range(F) for b in range(B)]


def test_fixture_shape(ghist):
    g = ghist
    assert (g["F"], g["B"], g["nodes"], len(g["node"])) == (3, 4, 2, 48)
    assert any(b == g["B"] for row in g["bins"] for b in row)           # a missing value
    assert any(v == -1 for v in g["node"])
    mem = cell_members(g)
    for name in ("labels", "floats"):
        case = g["cases"][name]
        assert case["counts"] == [len(m) for m in mem]
        assert [c is None for c in case["cells"]] == [not m for m in mem]
    # (feature 2, bin 3) is empty in both nodes
    assert mem[(0 * 3 + 2) * 4 + 3] == [] and mem[(1 * 3 + 2) * 4 + 3] == []
    assert set(g["cases"]["labels"]["e"]) == {0} and len(set(g["cases"]["floats"]["e"])) > 3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "paillier_golden_hist.json")) < 200 * 1024


@pytest.mark.parametrize("name", ["labels", "floats"])
def test_oracle_reproduces_cells(golden, ghist, name):
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    case = ghist["cases"][name]
    cs = [int(h, 16) for h in case["c"]]
    # the inputs are the reference's encryptions under golden_r
    if name == "labels":
        for i in (0, 17, 47):
            assert cs[i] == O.raw_encrypt(case["x"][i] % key.n, key, O.golden_r(key.n, 700, i))
    for s, mem in enumerate(cell_members(ghist)):
        if not mem:
            continue
        c, e = O.add_k([cs[i] for i in mem], [case["e"][i] for i in mem], key)
        assert [hex(c), e] == case["cells"][s], (name, s)
