#!/usr/bin/env python3
"""Key generation, host search against device search, in one process: generate_paillier_keypair for seeds 1..8 at
nb = 1024, 2048 and 4096, alternating the host path ($FLEXPAI_KEYGEN_GPU=0: _bigint.next_prime, the code before the
device search existed) and the device path (pai_next_prime: sieve, k_mr_w pass 1 and pass 2), each followed by the
key's Context and its first 1 000-element device-RNG encrypt, as HE_SA_FT does per exchange (tools/fresh_key_trace.py).
One untimed device search per size comes first (module load, the call's stream and scratch).

    python tools/gpu/keygen_ab.py [--seeds 8] [--sizes 1024,2048,4096] [--out profiles/keygen_ab.json]

Writes per-seed times, medians, the windows used and the kernel milliseconds of the two passes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen_ab.json"))
    a = ap.parse_args()
    from flex.crypto.paillier import _bigint, _native as N
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    x = np.random.default_rng(3).standard_normal(a.n).astype(np.float32)
    passes = {"p1": 0.0, "p2": 0.0, "l1": 0, "l2": 0}
    inner = N.next_prime_batch

    def counted(*args, **kw):
        out = inner(*args, **kw)
        t1, t2, l1, l2 = N.prime_last_times()
        passes["p1"] += t1
        passes["p2"] += t2
        passes["l1"] += l1
        passes["l2"] += l2
        return out

    N.next_prime_batch = counted

    def one(nb, seed, device):
        os.environ["FLEXPAI_KEYGEN_GPU"] = "1" if device else "0"
        for k in passes:
            passes[k] = 0
        s0 = N.prime_stats()
        t0 = time.perf_counter()
        pk, sk = generate_paillier_keypair(nb, seed=seed)
        t1 = time.perf_counter()
        c = N.Context(pk.n, 0, sk.p, sk.q)
        ct, ex, st = c.encrypt(x, rng_key=bytes(32), index_base=0)
        t2 = time.perf_counter()
        c.close()
        s1 = N.prime_stats()
        return {"seed": seed, "keygen_ms": round(1e3 * (t1 - t0), 3), "keygen_first_call_ms": round(1e3 * (t2 - t0), 3),
                "windows": s1["windows"] - s0["windows"], "device_searches": s1["device_searches"] - s0["device_searches"],
                "host_fallbacks": s1["host_fallbacks"] - s0["host_fallbacks"],
                "pass1_ms": round(passes["p1"], 3), "pass2_ms": round(passes["p2"], 3),
                "pass1_launches": passes["l1"], "pass2_launches": passes["l2"], "n": hex(pk.n)[:18]}

    result = {"elements_first_call": a.n, "sizes": {}}
    for nb in [int(v) for v in a.sizes.split(",")]:
        os.environ["FLEXPAI_KEYGEN_GPU"] = "1"
        if not _bigint.keygen_on_device(nb // 2):
            raise SystemExit(f"no device search for {nb // 2}-bit primes here")
        generate_paillier_keypair(nb, seed=1000)          # untimed: first use of this size's kernel
        host, dev = [], []
        for seed in range(1, a.seeds + 1):
            host.append(one(nb, seed, False))
            dev.append(one(nb, seed, True))
            assert host[-1]["n"] == dev[-1]["n"] and host[-1]["device_searches"] == 0 and dev[-1]["host_fallbacks"] == 0
        med = lambda rows, k: round(statistics.median(r[k] for r in rows), 3)   # noqa: E731
        row = {"default_window": 4 * (nb // 2), "host": host, "device": dev,
               "median_keygen_ms": {"host": med(host, "keygen_ms"), "device": med(dev, "keygen_ms")},
               "median_keygen_first_call_ms": {"host": med(host, "keygen_first_call_ms"),
                                               "device": med(dev, "keygen_first_call_ms")},
               "median_pass1_ms": med(dev, "pass1_ms"), "median_pass2_ms": med(dev, "pass2_ms"),
               "median_windows": med(dev, "windows")}
        row["device_below_half_host"] = row["median_keygen_ms"]["device"] < 0.5 * row["median_keygen_ms"]["host"]
        result["sizes"][str(nb)] = row
        print(json.dumps({k: v for k, v in row.items() if k not in ("host", "device")} | {"nb": nb}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
