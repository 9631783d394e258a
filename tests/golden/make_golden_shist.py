"""Golden vectors for encrypted histograms over a sparse bin matrix (pai_histogram_sparse) FROM THE REFERENCE: every cell
off its feature's default bin is the reference's own ``+`` chain over its stored members, and every default cell is
``T - S`` by the reference's operators: T the ``+`` chain over all samples of the node, S the chain over the node's stored
entries of the feature off the default bin (stored missing values included), and ``T + S * -1``.

Run in the survey container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_shist.py

40 samples, F = 5 features, B = 3 bins, 2 nodes, the keys of paillier_golden.json at 1024 and 2048 bits, float32 values
whose exponents differ inside a cell. The CSR matrix holds: feature 0 one-hot style (default bin 0, bins 1 and 2 stored,
some explicit default entries, one stored missing value), feature 1 with default_bin 7 (no default cell), feature 2
stored off the default bin for every sample but sample 5, whose row is empty (the default cell of the other node is
empty), feature 3 with no stored entry (the default cell is T), feature 4 with default bin 2; samples 3 and 20 carry
node -1.
"""
import functools
import json
import operator
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import enc_with_r, golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402


def matrix():
    N, F, B, nodes = 40, 5, 3, 2
    rng = np.random.default_rng(31)
    default_bin = [0, 7, 1, 0, 2]
    rows = []
    for i in range(N):
        row = {}
        if i != 5:
            if rng.random() < 0.5:
                row[0] = int(rng.integers(0, B))            # bin 0: an explicitly stored default entry
            if rng.random() < 0.6:
                row[1] = int(rng.integers(0, B))
            row[2] = int(rng.choice([0, 2]))                # never the default bin 1
            if rng.random() < 0.4:
                row[4] = int(rng.integers(0, B + 1))        # B: a missing value; 2: the default bin, stored
        rows.append(row)
    rows[9][0] = B                                          # a stored missing value of feature 0
    indptr, indices, data = [0], [], []
    for row in rows:
        for f in sorted(row):
            indices.append(f)
            data.append(row[f])
        indptr.append(len(indices))
    node = rng.integers(0, nodes, N).astype(np.int32)
    node[[3, 20]] = -1
    return N, F, B, nodes, default_bin, indptr, indices, data, node.tolist()


def main():
    N, F, B, nodes, default_bin, indptr, indices, data, node = matrix()
    out = {"generator": "tests/golden/make_golden_shist.py", "numpy": np.__version__, "cases": {}, "N": N, "F": F, "B": B,
           "nodes": nodes, "default_bin": default_bin, "indptr": indptr, "indices": indices, "data": data, "node": node}
    stored = [{indices[t]: data[t] for t in range(indptr[i], indptr[i + 1])} for i in range(N)]
    ct = lambda e: hex(e.ciphertext(be_secure=False))
    chain = lambda xs: functools.reduce(operator.add, xs)
    for nb in (1024, 2048):
        pe, _ = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pe.pub_key.n
        vals = (np.random.default_rng(nb).standard_normal(N) * 10.0 ** np.random.default_rng(nb + 1).integers(-5, 6, N)).astype(np.float32)
        enc = [enc_with_r(pe, float(v), golden_r(n, 900, i)) for i, v in enumerate(vals)]
        cells, counts = [], []
        for v in range(nodes):
            members = [i for i in range(N) if node[i] == v]
            for f in range(F):
                z = default_bin[f]
                for b in range(B):
                    if b != z:
                        mem = [i for i in members if stored[i].get(f) == b]
                        counts.append(len(mem))
                        cells.append([ct(chain([enc[i] for i in mem])), int(chain([enc[i] for i in mem]).exponent)] if mem else None)
                        continue
                    rest = [i for i in members if f in stored[i] and stored[i][f] != z]
                    counts.append(len(members) - len(rest))
                    if len(members) == len(rest):
                        cells.append(None)
                        continue
                    acc = chain([enc[i] for i in members])
                    if rest:
                        acc = acc + chain([enc[i] for i in rest]) * -1
                    cells.append([ct(acc), int(acc.exponent)])
        out["cases"][str(nb)] = {"c": [ct(e) for e in enc], "e": [int(e.exponent) for e in enc],
                                 "x": [float(v).hex() for v in vals], "cells": cells, "counts": counts}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_shist.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_shist.json")


if __name__ == "__main__":
    main()
