"""Golden vectors for packed plaintexts (pai_encrypt_packed / pai_decrypt_packed) FROM THE REFERENCE.

Run where the reference is installed only (it never travels to the GPU box), with the reference on PYTHONPATH and the
interpreter make_golden.py names (gmpy2 2.0.8, numpy 1.26):

    python3.9 tests/golden/make_golden_packed.py

The reference has no packing, so the pack is restated here in three lines (the package and the reference share the
name `flex`, so the package's own cannot be imported next to it): M = sum_j t_j 2^(sb j), a signed integer. Everything
else is the reference's own code on the keys of paillier_golden.json: raw_encrypt(M mod n, pk, r) under
make_golden.golden_r, the 3-way sum of the ciphertexts through PaillierEncryptedNumber.__add__, the product of the
first one by -3 through __mul__ (the invert branch, encrypted_number.py:97-101), and the raw decryption of each.
Per key size two layouts (slot_bits, value_bits, exponent) at the maximum slot count, three ciphertexts each: random
slots, every slot at -max, and slots alternating between +max and -max.
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

LAYOUTS = {1024: [(32, 24, 5), (64, 53, 10)], 2048: [(32, 24, 5), (64, 53, 10)], 4096: [(40, 33, 7), (56, 50, 9)]}
SEED_R = 800


def pack(ts, sb):
    M = 0
    for j, t in enumerate(ts):
        M += int(t) << (sb * j)
    return M


def main():
    import gmpy2
    out = {"generator": "tests/golden/make_golden_packed.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "gmpy2": gmpy2.version(), "cases": {}}
    for nb in (1024, 2048, 4096):
        pk, sk = generate_paillier_keypair(nb, seed=1)
        pe, pd = generate_paillier_encryptor_decryptor(nb, seed=1)
        n = pk.n
        assert pe.pub_key.n == n
        raw_decrypt = pd._PaillierDecryptor__raw_decrypt
        recs = []
        for li, (sb, vb, e) in enumerate(LAYOUTS[nb]):
            k = (nb - 2) // sb
            mx = (1 << (vb - 1)) - 1
            rng = np.random.default_rng(nb + li)
            slots = [[int(v) for v in rng.integers(-mx, mx + 1, k)], [-mx] * k, [mx if j % 2 == 0 else -mx for j in range(k)]]
            rs = [golden_r(n, SEED_R + li, i) for i in range(3)]
            cts = [int(raw_encrypt(pack(ts, sb) % n, pk, r)) for ts, r in zip(slots, rs)]
            nums = [PaillierEncryptedNumber(pk, c, e) for c in cts]
            s3 = nums[0] + nums[1] + nums[2]
            m3 = nums[0] * -3
            assert s3.exponent == e and m3.exponent == e
            c_sum, c_mul = int(s3.ciphertext(be_secure=False)), int(m3.ciphertext(be_secure=False))
            recs.append({"slot_bits": sb, "value_bits": vb, "exponent": e, "slots": k,
                         "t": slots, "r": [hex(int(r)) for r in rs], "ct": [hex(c) for c in cts],
                         "sum3": hex(c_sum), "mul_m3": hex(c_mul),
                         "raw": [hex(int(raw_decrypt(c))) for c in cts],
                         "raw_sum3": hex(int(raw_decrypt(c_sum))), "raw_mul_m3": hex(int(raw_decrypt(c_mul)))})
        out["cases"][str(nb)] = recs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_packed.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_packed.json")


if __name__ == "__main__":
    main()
