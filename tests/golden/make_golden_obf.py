"""Golden vectors for the re-randomisation of existing ciphertexts (PaillierEncryptedNumber.apply_obfuscation over
arrays: pai_obfuscate) FROM THE REFERENCE.

Run where the reference is installed only (it never travels to the GPU box), with the reference on PYTHONPATH and the
interpreter make_golden.py names (gmpy2 2.0.8, numpy 1.26):

    python3.9 tests/golden/make_golden_obf.py

Every expected value is the reference's own ``apply_obfuscation(c, pub_key, r)`` (obfuscator.py:23-37: c * r^n mod
n^2) on the keys of paillier_golden.json. Inputs: fresh encryptions under make_golden.golden_r, an 8-way sum
(__raw_add results are the ciphertexts that are not obfuscated yet), products by a negative float (the invert branch
of __mul__, encrypted_number.py:97-101) and the edge values c = 1, n^2 - 1 and 12345 p. Every input meets an r from
golden_r; the first five also meet r = 1, 2, n - 1, n + 1 and n^2 - 1 in turn.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import enc_with_r, golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402
from flex.crypto.paillier.keypair import generate_paillier_keypair  # noqa: E402
from flex.crypto.paillier.obfuscator import apply_obfuscation  # noqa: E402

N_FRESH = 13
SEED_IN, SEED_SUM, SEED_OBF = 700, 710, 720


def main():
    import gmpy2
    out = {"generator": "tests/golden/make_golden_obf.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "gmpy2": gmpy2.version(), "cases": {}}
    for nb in (1024, 2048, 4096):
        pk, sk = generate_paillier_keypair(nb, seed=1)
        pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pk.n
        assert pe.pub_key.n == n
        p = min(sk.p, sk.q)
        xs = (np.random.default_rng(nb + 3).standard_normal(N_FRESH) * 3.0).astype(np.float64)
        fresh = [enc_with_r(pe, v, golden_r(n, SEED_IN, i)) for i, v in enumerate(xs)]
        inputs = [("fresh", e.ciphertext(be_secure=False)) for e in fresh]
        acc = enc_with_r(pe, np.float64(0.5), golden_r(n, SEED_SUM, 0))
        for k in range(1, 8):
            acc = acc + enc_with_r(pe, np.float64(0.25 * k - 1.0), golden_r(n, SEED_SUM, k))
        inputs.append(("sum8", acc.ciphertext(be_secure=False)))
        for j, s in enumerate((-0.75, -1234.5)):
            inputs.append(("mul_neg", (fresh[j] * s).ciphertext(be_secure=False)))
        inputs += [("one", 1), ("nsq_minus_1", n * n - 1), ("multiple_of_p", 12345 * p)]
        special = [1, 2, n - 1, n + 1, n * n - 1]
        recs = []
        for i, (kind, c) in enumerate(inputs):
            rs = [golden_r(n, SEED_OBF, i)] + ([special[i]] if i < len(special) else [])
            for r in rs:
                recs.append({"kind": kind, "c": hex(int(c)), "r": hex(int(r)),
                             "out": hex(int(apply_obfuscation(int(c), pk, int(r))))})
        out["cases"][str(nb)] = recs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_obf.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_obf.json")


if __name__ == "__main__":
    main()
