#!/usr/bin/env python3
"""Golden vectors for pai_repack (packed ciphertexts folded into fuller ones) FROM THE REFERENCE.

Run on the CPU, where the reference is installed only (it never travels to the GPU box), with the interpreter
tests/golden/make_golden.py names (gmpy2 2.0.8, numpy 1.26) and the reference's path as the argument:

    python3.9 tools/make_golden_repack.py /path/to/reference

Everything is the reference's own code on the keys of tests/golden/paillier_golden.json. Per key size (1024 and 2048
bits) three cases (slot_bits sb, slots per input s, the largest g with s g <= (nb - 2) // sb): g + 2 packed inputs -- a
full output and a ragged one of two inputs -- whose s g + 2 s slots hold signed integers up to +-(2^(sb - 1) - 1), the
extremes among them. Input i is PaillierEncryptedNumber(pk, raw_encrypt(M_i mod n, pk, r_i), 0) with
M_i = sum_u t_(i s + u) 2^(sb u) and r_i = make_golden.golden_r(n, 910 + case, i). Output c is the reference's own

    sum(c_j * (1 << (s * sb * j)) for j in range(inputs of c))

through PaillierEncryptedNumber.__mul__ and __add__ at exponent 0, and the raw decryption of that sum. Writes
tests/golden/paillier_golden_repack.json.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((48, 2), (24, 3), (64, 1))                         # (sb, s): strides 96, 72 and 64
SEED_R = 910


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "flex")):
        sys.exit(__doc__)
    sys.path[:0] = [sys.argv[1], os.path.join(ROOT, "tests", "golden")]
    import gmpy2
    from make_golden import golden_r
    from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    from flex.crypto.paillier.raw_encrypt import raw_encrypt
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    out = {"generator": "tools/make_golden_repack.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "gmpy2": gmpy2.version(), "cases": {}}
    for nb in (1024, 2048):
        pk, sk = generate_paillier_keypair(nb, seed=1)
        pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pk.n
        assert pe.pub_key.n == n == int(keys[str(nb)]["n"], 16)
        raw_decrypt = pd._PaillierDecryptor__raw_decrypt
        recs = []
        for case, (sb, s) in enumerate(CASES):
            g = (nb - 2) // sb // s
            N = g + 2
            mx = (1 << (sb - 1)) - 1
            rng = np.random.default_rng(nb + sb + s)
            ts = [int(v) for v in rng.integers(-mx, mx, N * s, endpoint=True)]
            for i in range(0, N * s, 3):
                ts[i] = mx if i % 2 == 0 else -mx
            Ms = [sum(t << (sb * u) for u, t in enumerate(ts[i * s:(i + 1) * s])) for i in range(N)]
            cts = [int(raw_encrypt(M % n, pk, golden_r(n, SEED_R + case, i))) for i, M in enumerate(Ms)]
            nums = [PaillierEncryptedNumber(pk, c, 0) for c in cts]
            repacked, raws = [], []
            for c in range(0, N, g):
                row = nums[c:c + g]
                acc = row[0] * 1
                for j in range(1, len(row)):
                    acc = acc + row[j] * (1 << (s * sb * j))
                assert acc.exponent == 0
                v = int(acc.ciphertext(be_secure=False))
                repacked.append(hex(v))
                raws.append(hex(int(raw_decrypt(v))))
            recs.append({"slot_bits": sb, "slots": s, "group": g, "t": ts, "ct": [hex(c) for c in cts],
                         "repacked": repacked, "raw": raws})
        out["cases"][str(nb)] = recs
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden_repack.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote tests/golden/paillier_golden_repack.json")


if __name__ == "__main__":
    main()
