"""Golden vectors for encrypted histograms (pai_histogram: the per-bin sums of IV_FFS,
flex/tools/feature_iv_algo/hetero_bin.py:27-36, over every feature at once, and the (node, feature, bin) sums of
gradient boosting) FROM THE REFERENCE: every non-empty cell is the reference's own ``+`` chain over its members.

Run in the survey container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_hist.py

48 samples, F = 3 features, B = 4 bins, 2 nodes. One bin id equals B (a missing value), (feature 2, bin 3) is empty in
both nodes, and some samples carry node -1. Labels are 0/1 ints (exponent 0, as IV_FFS encrypts them); the float32 case
has exponents that differ inside a cell.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import enc_with_r, golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402


def main():
    out = {"generator": "tests/golden/make_golden_hist.py", "numpy": np.__version__, "cases": {}}
    nb, N, F, B, nodes = 1024, 48, 3, 4, 2
    pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
    n = pe.pub_key.n
    rng = np.random.default_rng(23)
    bins = rng.integers(0, B, (N, F)).astype(np.uint8)
    bins[:, 2] = rng.integers(0, B - 1, N)         # (feature 2, bin 3) stays empty
    bins[7, 1] = B                                  # missing
    node = rng.integers(0, nodes, N).astype(np.int32)
    node[[3, 20, 41]] = -1
    labels = rng.integers(0, 2, N).astype(np.int64)
    floats = (rng.standard_normal(N) * 10.0 ** rng.integers(-6, 7, N)).astype(np.float32)
    ct = lambda e: hex(e.ciphertext(be_secure=False))
    for name, vals in (("labels", labels), ("floats", floats)):
        enc = [enc_with_r(pe, (int(v) if name == "labels" else float(v)), golden_r(n, 700, i)) for i, v in enumerate(vals)]
        cells, counts = [], []
        for v in range(nodes):
            for f in range(F):
                for b in range(B):
                    mem = [i for i in range(N) if node[i] == v and bins[i, f] == b]
                    counts.append(len(mem))
                    if not mem:
                        cells.append(None)
                        continue
                    acc = enc[mem[0]]
                    for i in mem[1:]:
                        acc = acc + enc[i]
                    cells.append([ct(acc), int(acc.exponent)])
        out["cases"][name] = {"c": [ct(e) for e in enc], "e": [int(e.exponent) for e in enc],
                              "x": [int(v) if name == "labels" else float(v).hex() for v in vals],
                              "cells": cells, "counts": counts}
    out["bins"] = bins.tolist()
    out["node"] = node.tolist()
    out["F"], out["B"], out["nodes"] = F, B, nodes
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_hist.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_hist.json")


if __name__ == "__main__":
    main()
