#!/usr/bin/env python3
"""A/B of the 4096-bit public-key encryption of a party without the private key, in one process on one GPU:
a = the product library's pair-group chain (kernels_pe4.hpp: k_pe4_pre / k_pe4_pow / k_pe4_fin),
b = the test build under $FLEXPAI_PAIR=0, i.e. k_encrypt<8> (the kernel the chain replaces, unchanged),
on 262 144 float32 elements (device-resident, device RNG, rows_max 0, public fixed bases off). One warm-up call each,
then three rounds that alternate a and b; every timing ends in a device synchronise. Writes the rates, their spread,
a's stage times, k_pe4_pow's lane-MAC count and rate, and the libraries' sha256 to profiles/pe4_ab.json (--out), and
prints the same JSON line.

    python tools/pe4_ab.py [--n 262144] [--rounds 3] [--out profiles/pe4_ab.json]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402

S = 152                      # limbs of n on the pair groups (kernels_pe4.hpp)
INT_MAC_PEAK = 35.13e12      # lane-MACs/s: the integer multiply-add peak DESIGN.md uses


def chain_ops(e: int):
    """(squares, products) of k_pe4_pow for the exponent e: flexpai.hip's sliding_schedule (window 5, left to right)
    behind build_lane_program's table (one square, 15 products), plus the final product with c0."""
    K = 5
    bit = lambda i: (e >> i) & 1   # noqa: E731
    i = e.bit_length() - 1
    lo = max(i - K + 1, 0)
    while not bit(lo):
        lo += 1
    i = lo - 1
    sq, mul = 1, 15 + 1
    while i >= 0:
        if not bit(i):
            sq += 1
            i -= 1
            continue
        lo = max(i - K + 1, 0)
        while not bit(lo):
            lo += 1
        sq += i - lo + 1
        mul += 1
        i = lo - 1
    return sq, mul


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pe4_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        key_n = int(json.load(f)["keys"]["4096"]["n"], 16)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.n
    x = torch.randn(n, dtype=torch.float32, device=dev)
    ex = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    side = {}
    for name in ("a", "b"):
        os.environ["FLEXPAI_PAIR"] = "1" if name == "a" else "0"
        lib = N.load_library() if name == "a" else N.load_library(N.XCHECK_LIB_PATH)
        c = N.Context(key_n, 0, lib=None if name == "a" else lib)
        c.set_rows_max(0)
        c.set_public_fixed_base(False)
        c.set_stage_timing(True)
        side[name] = (lib, c, torch.empty((n, c.ct_words), dtype=torch.int32, device=dev))
    assert side["a"][1].pair_paths & 4 and not side["b"][1].pair_paths & 4

    def call(name):
        lib, c, ct = side[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.pai_encrypt_dev(c.handle, N.PAI_F32, x.data_ptr(), n, 0, 0, N.PAI_OBF_RNG, None, 0, 0, bytes(range(32)), 0,
                                 ct.data_ptr(), ex.data_ptr(), st.data_ptr(), stream.cuda_stream)
        assert rc == 0, lib.pai_last_error()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name in ("a", "b"):
        call(name)                                   # warm-up: scratch and work buffers, code objects
    times = {"a": [], "b": []}
    stages = []
    for _ in range(args.rounds):
        for name in ("a", "b"):
            times[name].append(call(name))
            if name == "a":
                stages.append(side["a"][1].stage_times())
    row = {"nb": 4096, "n": n, "rounds": args.rounds,
           "identical": bool(torch.equal(side["a"][2], side["b"][2]))}
    for name in ("a", "b"):
        ms = [t * 1e3 for t in times[name]]
        med = statistics.median(ms)
        row[name] = {"ms": [round(v, 2) for v in ms], "median_ms": round(med, 2),
                     "encrypts_per_s": round(n / med * 1e3),
                     "spread": round((max(ms) - min(ms)) / med, 4)}
    row["ratio_a_over_b"] = round(row["a"]["encrypts_per_s"] / row["b"]["encrypts_per_s"], 3)
    row["a"]["stages_ms"] = [[round(v, 2) for v in s] for s in stages]     # k_pe4_pre, k_pe4_pow, k_pe4_fin per round
    sq, mul = chain_ops(key_n)
    macs = (4 * sq + 5 * mul) * S * S
    pow_ms = statistics.median(s[1] for s in stages)
    row["k_pe4_pow"] = {"squares": sq, "products": mul, "lane_macs_per_element": macs,
                        "lane_macs_per_s": round(macs * n / pow_ms * 1e3),
                        "share_of_int_mac_peak": round(macs * n / pow_ms * 1e3 / INT_MAC_PEAK, 4)}
    row["sha256"] = {"libflexpai.so": sha256(N.LIB_PATH), "libflexpai_xcheck.so": sha256(N.XCHECK_LIB_PATH)}
    row["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
