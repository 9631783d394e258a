"""Golden vectors for pai_pack_ciphertexts (existing ciphertexts folded into packed ones) FROM THE REFERENCE.

Run where the reference is installed only (it never travels to the GPU box), with the reference on PYTHONPATH and the
interpreter make_golden.py names (gmpy2 2.0.8, numpy 1.26):

    python3.9 tests/golden/make_golden_fold.py

Everything is the reference's own code on the keys of paillier_golden.json. Per key size one layout (slot_bits, E, k)
-- the maximum slot count at 1024 and 2048 bits, 8 slots at 4096 bits, where a ciphertext is 2 KB of hex and the full
102 slots would make the fixture megabytes -- and 2k + 1 integers t_i, each held at an exponent e_i = E - D_i with
D_i in {0, 1, 2}: PaillierEncryptedNumber(pk, raw_encrypt(t_i mod n, pk, r_i), e_i) under make_golden.golden_r, so the
value is t_i 16^-e_i and its slot integer at E is t_i 16^D_i. Output c is the reference's own

    sum(c_j * (1 << (slot_bits * j)) for j in range(slots of c))

through PaillierEncryptedNumber.__mul__ and __add__ (its alignment to the largest exponent, which is E in every output
here: slot 0 of each output has D = 0), and the raw decryption of that sum.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402
from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber  # noqa: E402
from flex.crypto.paillier.keypair import generate_paillier_keypair  # noqa: E402
from flex.crypto.paillier.raw_encrypt import raw_encrypt  # noqa: E402

LAYOUTS = {1024: (32, 5, 31), 2048: (64, 5, 31), 4096: (40, 7, 8)}     # (slot_bits, E, slots)
T_BITS = 20                                                 # |t_i| < 2^20: t_i 16^2 stays far inside a slot
SEED_R = 900


def main():
    import gmpy2
    out = {"generator": "tests/golden/make_golden_fold.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "gmpy2": gmpy2.version(), "cases": {}}
    for nb in (1024, 2048, 4096):
        pk, sk = generate_paillier_keypair(nb, seed=1)
        pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pk.n
        assert pe.pub_key.n == n
        raw_decrypt = pd._PaillierDecryptor__raw_decrypt
        sb, E, k = LAYOUTS[nb]
        assert k <= (nb - 2) // sb
        N = 2 * k + 1
        rng = np.random.default_rng(nb + 77)
        ts = [int(v) for v in rng.integers(-(1 << T_BITS) + 1, 1 << T_BITS, N)]
        ds = [int(v) for v in rng.integers(0, 3, N)]
        for c in range(0, N, k):
            ds[c] = 0                                       # the largest exponent of every output is E
        ds[k - 1], ds[2 * k - 1] = 2, 1                     # shifted top slots
        rs = [golden_r(n, SEED_R, i) for i in range(N)]
        cts = [int(raw_encrypt(t % n, pk, r)) for t, r in zip(ts, rs)]
        nums = [PaillierEncryptedNumber(pk, c, E - d) for c, d in zip(cts, ds)]
        folded, raws = [], []
        for c in range(0, N, k):
            row = nums[c:c + k]
            s = row[0] * 1
            for j in range(1, len(row)):
                s = s + row[j] * (1 << (sb * j))
            assert s.exponent == E
            v = int(s.ciphertext(be_secure=False))
            folded.append(hex(v))
            raws.append(hex(int(raw_decrypt(v))))
        out["cases"][str(nb)] = {"slot_bits": sb, "exponent": E, "slots": k, "t": ts, "delta": ds,
                                 "ct": [hex(c) for c in cts], "folded": folded, "raw": raws}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_fold.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_fold.json")


if __name__ == "__main__":
    main()
