"""Golden vectors for prefix sums of ciphertext arrays (pai_cumsum: the split candidates G_L(b) of a boosting
histogram, the cumulative good / bad counts of IV_FFS binning) FROM THE REFERENCE: numpy's object loop over
PaillierEncryptedNumber, one ``__add__`` per element.

Run in the survey container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_cumsum.py

A (3, 9) array under the 1024-bit key (seed 1). Labels are 0/1 ints (every exponent 0); the float32 case spreads over
10^+-6, so exponents differ inside a row and the running maximum rises mid-row. Per case: ``np.cumsum`` along axis 0 and
axis 1 and the flipped scans (the cumsum of the flipped axis, flipped back). The scan along axis 1 is stored in full;
the other three as the SHA-256 of "<ciphertext hex>:<exponent>" per element, which pins the same bits in a quarter of
the space.
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import enc_with_r, golden_r  # noqa: E402

from flex.crypto.paillier.api import generate_paillier_encryptor_decryptor  # noqa: E402

SHAPE = (3, 9)


def digest(c_hex: str, e: int) -> str:
    return hashlib.sha256(f"{c_hex}:{e}".encode()).hexdigest()


def main():
    out = {"generator": "tests/golden/make_golden_cumsum.py", "numpy": np.__version__, "shape": list(SHAPE), "cases": {}}
    pe, pd = generate_paillier_encryptor_decryptor(1024, seed=1)
    n = pe.pub_key.n
    N = SHAPE[0] * SHAPE[1]
    rng = np.random.default_rng(29)
    labels = rng.integers(0, 2, N).astype(np.int64)
    floats = (rng.standard_normal(N) * 10.0 ** rng.integers(-6, 7, N)).astype(np.float32)
    ct = lambda e: hex(e.ciphertext(be_secure=False))
    for name, vals in (("labels", labels), ("floats", floats)):
        enc = [enc_with_r(pe, (int(v) if name == "labels" else float(v)), golden_r(n, 900, i)) for i, v in enumerate(vals)]
        arr = np.array(enc, dtype=object).reshape(SHAPE)
        case = {"c": [ct(e) for e in enc], "e": [int(e.exponent) for e in enc],
                "x": [int(v) if name == "labels" else float(v).hex() for v in vals]}
        for axis in (0, 1):
            fwd = np.cumsum(arr, axis)
            rev = np.flip(np.cumsum(np.flip(arr, axis), axis), axis)
            for tag, res in ((f"axis{axis}", fwd), (f"axis{axis}_rev", rev)):
                assert res.shape == SHAPE
                flat = res.reshape(-1)
                if tag == "axis1":
                    case[tag] = [[ct(e), int(e.exponent)] for e in flat]
                else:
                    case[tag + "_sha256"] = [digest(ct(e), int(e.exponent)) for e in flat]
        out["cases"][name] = case
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_golden_cumsum.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote paillier_golden_cumsum.json")


if __name__ == "__main__":
    main()
