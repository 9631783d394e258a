"""The re-randomisation fixture (tests/golden/paillier_golden_obf.json, from the reference's apply_obfuscation) against
the CPU oracle, and the C ABI's declarations. No GPU."""
import json
import os
import re

import pytest

from oracle import paillier_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_obf():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_obf.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("nb", [1024, 2048, 4096])
def test_fixture_reproduces_from_oracle(golden, golden_obf, nb):
    k = golden["keys"][str(nb)]
    key = O.Key(int(k["n"], 16), int(k["p"], 16), int(k["q"], 16))
    recs = golden_obf["cases"][str(nb)]
    assert len(recs) >= 20
    for i, rec in enumerate(recs):
        c, r = int(rec["c"], 16), int(rec["r"], 16)
        assert 0 < c < key.nsquare and 0 < r < key.nsquare
        assert c * pow(r, key.n, key.nsquare) % key.nsquare == int(rec["out"], 16), (nb, i, rec["kind"])


def test_fixture_covers_the_issue_cases(golden, golden_obf):
    assert golden_obf["gmpy2"] and golden_obf["numpy"] and golden_obf["generator"].endswith("make_golden_obf.py")
    for nb in (1024, 2048, 4096):
        k = golden["keys"][str(nb)]
        n, p = int(k["n"], 16), int(k["p"], 16)
        recs = golden_obf["cases"][str(nb)]
        kinds = {r["kind"] for r in recs}
        assert kinds == {"fresh", "sum8", "mul_neg", "one", "nsq_minus_1", "multiple_of_p"}
        cs = {int(r["c"], 16) for r in recs}
        assert {1, n * n - 1} <= cs and any(c % p == 0 or c % (n // p) == 0 for c in cs)
        assert {1, 2, n - 1, n + 1, n * n - 1} <= {int(r["r"], 16) for r in recs}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "paillier_golden_obf.json")) < 300 * 1024


def test_header_declares_both_symbols():
    header = open(os.path.join(ROOT, "include", "flexpai.h")).read()
    declared = set(re.findall(r"^\s*int\s+(pai_\w+)\s*\(", header, re.M))
    assert {"pai_obfuscate", "pai_obfuscate_dev"} <= declared
    assert re.search(r"#define\s+PAI_OPT_OBF_CHUNK\s+18\b", header)
    from flex.crypto.paillier import _native
    assert {"pai_obfuscate", "pai_obfuscate_dev"} <= set(_native.EXPORTED)
    assert _native.PAI_OPT_OBF_CHUNK == 18
