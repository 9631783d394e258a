"""Golden vectors for segmented weighted sums (pai_segment_dot: out_s = sum_t c[index[t]] * x[t]) FROM THE REFERENCE.

Run where the reference is installed only (it never travels to the GPU box), with the reference on PYTHONPATH and the
interpreter make_golden.py names (gmpy2 2.0.8, numpy 1.26):

    python3.9 tests/golden/make_golden_segdot.py

Per key size (the keys of paillier_golden.json at 1024 and 2048 bits) 24 ciphertexts: the reference's encryption, under
make_golden.golden_r, of ints and of floats of mixed magnitude, so the exponents are mixed. The 70 entries form
segments of 0, 1, 15, 16, 17 and 21 entries with repeated indices; one weight set is float64 (negatives, +0.0, -0.0, tiny
and large magnitudes), one int64. Output s is the reference's own

    c[i0] * x0 + c[i1] * x1 + ...

through PaillierEncryptedNumber.__mul__ and __add__, recorded as ciphertext, exponent and decrypted value; an empty
segment is null.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import enc_with_r, golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402

NCT = 24
LENS = (0, 1, 15, 16, 17, 21)
SEED_R = 1100


def main():
    import gmpy2
    out = {"generator": "tests/golden/make_golden_segdot.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "gmpy2": gmpy2.version(), "cases": {}}
    for nb in (1024, 2048):
        pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pe.pub_key.n
        rng = np.random.default_rng(nb + 5)
        plain = []
        for i in range(NCT):
            if i % 3 == 0:
                plain.append(int(rng.integers(-1000, 1000)))                      # exponent 0
            else:
                plain.append(float(rng.standard_normal() * 10.0 ** int(rng.integers(-6, 7))))
        enc = [enc_with_r(pe, v, golden_r(n, SEED_R, i)) for i, v in enumerate(plain)]
        nnz = sum(LENS)
        index = [int(v) for v in rng.integers(0, NCT, nnz)]
        index[2], index[3], index[20] = index[1], index[1], index[1]              # repeats inside and across segments
        seg_off = [int(v) for v in np.concatenate([[0], np.cumsum(LENS)])]
        wf = [float(v) for v in rng.standard_normal(nnz) * 10.0 ** rng.integers(-4, 5, nnz)]
        wf[5], wf[6], wf[17], wf[40] = 0.0, -0.0, 1.0, -1.0
        wf[33] = 0.0                                                              # a stored zero inside a long segment
        wi = [int(v) for v in rng.integers(-50, 51, nnz)]
        wi[7], wi[18] = 0, -1
        case = {"plain": [v if isinstance(v, int) else float(v).hex() for v in plain],
                "c": [hex(e.ciphertext(be_secure=False)) for e in enc], "e": [int(e.exponent) for e in enc],
                "index": index, "seg_off": seg_off, "weights": {}, "out": {}}
        for name, ws in (("f64", wf), ("i64", wi)):
            res = []
            for s in range(len(LENS)):
                acc = None
                for t in range(seg_off[s], seg_off[s + 1]):
                    term = enc[index[t]] * ws[t]
                    acc = term if acc is None else acc + term
                res.append(None if acc is None else
                           [hex(acc.ciphertext(be_secure=False)), int(acc.exponent), float(pd.decrypt(acc)).hex()])
            case["weights"][name] = [float(w).hex() for w in ws] if name == "f64" else ws
            case["out"][name] = res
        out["cases"][str(nb)] = case
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_segdot.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_segdot.json")


if __name__ == "__main__":
    main()
