"""The prefix-sum fixture (tests/golden/paillier_golden_cumsum.json, the reference's np.cumsum over
PaillierEncryptedNumber) against the CPU oracle: oracle.add_k over each prefix reproduces every stored (ciphertext,
exponent), in full along axis 1 and through the stored SHA-256 digests for axis 0 and the flipped scans."""
import hashlib
import json
import os

import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "paillier_golden_cumsum.json")
TAGS = [("axis0", 0, False), ("axis0_rev", 0, True), ("axis1", 1, False), ("axis1_rev", 1, True)]


@pytest.fixture(scope="module")
def gcs():
    with open(PATH) as f:
        return json.load(f)


def matches(case, tag, flat):
    """flat: [(ciphertext int, exponent)] in array order against the stored scan `tag`."""
    if tag in case:
        return [[hex(c), e] for c, e in flat] == case[tag]
    return [hashlib.sha256(f"{hex(c)}:{e}".encode()).hexdigest() for c, e in flat] == case[tag + "_sha256"]


def prefixes(shape, axis, rev):
    """For every flat position of a C-contiguous array: the flat positions of its prefix (suffix) along `axis`."""
    R, C = shape
    out = []
    for r in range(R):
        for c in range(C):
            if axis == 0:
                js = range(r, R) if rev else range(0, r + 1)
                out.append([j * C + c for j in js])
            else:
                js = range(c, C) if rev else range(0, c + 1)
                out.append([r * C + j for j in js])
    return out


def test_fixture_shape(gcs):
    assert gcs["shape"] == [3, 9] and set(gcs["cases"]) == {"labels", "floats"}
    for case in gcs["cases"].values():
        assert len(case["c"]) == len(case["e"]) == 27 and len(case["axis1"]) == 27
        for tag in ("axis0", "axis0_rev", "axis1_rev"):
            assert len(case[tag + "_sha256"]) == 27
    assert set(gcs["cases"]["labels"]["e"]) == {0} and len(set(gcs["cases"]["floats"]["e"])) > 3
    # the running maximum rises inside a row of the float case
    ex = [e for _, e in gcs["cases"]["floats"]["axis1"]]
    assert any(ex[r * 9 + j] < ex[r * 9 + j + 1] for r in range(3) for j in range(8))
    assert os.path.getsize(PATH) < 150 * 1024


@pytest.mark.parametrize("name", ["labels", "floats"])
def test_oracle_reproduces_the_scans(golden, gcs, name):
    k = golden["keys"]["1024"]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    case = gcs["cases"][name]
    cs = [int(h, 16) for h in case["c"]]
    if name == "labels":                                   # the inputs are the reference's encryptions under golden_r
        for i in (0, 13, 26):
            assert cs[i] == O.raw_encrypt(case["x"][i] % key.n, key, O.golden_r(key.n, 900, i))
    for tag, axis, rev in TAGS:
        flat = [O.add_k([cs[i] for i in mem], [case["e"][i] for i in mem], key) for mem in prefixes((3, 9), axis, rev)]
        assert matches(case, tag, flat), (name, tag)
