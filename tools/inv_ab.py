#!/usr/bin/env python3
"""A/B of the batch inversion behind negative scalars, in one process on one GPU:
a = this tree's library (the pyramid stops at 64 values, inverted by k_modinv, kernels_inv.hpp),
b = a library built from the parent commit (--parent: levels down to one value, inverted on the host; without one,
    this tree's library with PAI_OPT_INV_DEVICE = 0, which runs that code unchanged -- recorded as "b_kind").
Calls: pai_mul_dev by the integer -1 at 1 000 and 262 144 ciphertexts at 1024, 2048 and 4096 bits, and one
pai_matmul_dev of shape (1, 4096, 64) at 2048 bits (DESIGN.md section 8 item 9's table). Ciphertexts are random residues
mod n^2. One warm-up call per side, then --rounds rounds that alternate a and b; every call is timed by HIP events on
the current stream. Side a's pai_neg_dev at 4 values (one level: k_inv_up, k_modinv, k_inv_down) is timed the same way
as the closest figure to k_modinv's own time, next to the registers and occupancy the runtime reports. Writes the times,
their spread and whether the outputs are identical to --out, and prints the same JSON.

    python tools/inv_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--out profiles/inv_ab.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 262144])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inv_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib_a = N.load_library(N.LIB_PATH)
    have_parent = os.path.exists(args.parent)
    lib_b = N.load_library(args.parent) if have_parent else lib_a
    result = {"b_kind": "parent library" if have_parent else "same library, PAI_OPT_INV_DEVICE = 0", "rounds": args.rounds,
              "device": torch.cuda.get_device_name(dev), "unit": "ms", "cases": [], "k_modinv": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def ab(label, calls, outs):
        for s in "ab":
            calls[s]()                                         # warm-up: buffers, code objects
        ms = {"a": [], "b": []}
        for _ in range(args.rounds):
            for s in "ab":
                ms[s].append(timed(calls[s]))
        row = {"case": label, "identical": bool(torch.equal(outs["a"], outs["b"]))}
        for s in "ab":
            row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(statistics.median(ms[s]), 3),
                      "spread_ms": round(max(ms[s]) - min(ms[s]), 3)}
        row["a_slower_beyond_spread"] = bool(min(ms["a"]) > max(ms["b"]))
        result["cases"].append(row)
        print(json.dumps(row), flush=True)

    minus1 = torch.tensor([-1], dtype=torch.int64, device=dev)
    for nb in (1024, 2048, 4096):
        n = int(keys[str(nb)]["n"], 16)
        side = {"a": (lib_a, N.Context(n, 0, lib=lib_a)), "b": (lib_b, N.Context(n, 0, lib=lib_b))}
        if not have_parent:
            side["b"][1].set_inv_device(False)
        W = side["a"][1].ct_words
        g = torch.Generator(device=dev).manual_seed(nb)

        def residues(count):
            ct = torch.randint(0, 2 ** 31 - 1, (count, W), dtype=torch.int32, device=dev, generator=g)
            ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
            return ct

        for size in args.sizes:
            ct, ex = residues(size), torch.zeros(size, dtype=torch.int32, device=dev)
            outs = {s: torch.empty((size, W), dtype=torch.int32, device=dev) for s in "ab"}
            oe, st = torch.empty(size, dtype=torch.int32, device=dev), torch.empty(size, dtype=torch.int32, device=dev)

            def mul(s, ct=ct, ex=ex, outs=outs, oe=oe, st=st, size=size):
                lib, c = side[s]
                rc = lib.pai_mul_dev(c._h, ct.data_ptr(), ex.data_ptr(), size, N.PAI_I64, minus1.data_ptr(), 0,
                                     outs[s].data_ptr(), oe.data_ptr(), st.data_ptr(), stream.cuda_stream)
                assert rc == 0, lib.pai_last_error()
            ab(f"pai_mul_dev x -1, {nb} bits, {size}", {s: (lambda s=s: mul(s)) for s in "ab"}, outs)
        if nb == 2048:
            m, K, d = 1, 4096, 64
            ct, ex = residues(m * K), torch.zeros(m * K, dtype=torch.int32, device=dev)
            x = torch.randn((K, d), dtype=torch.float64, device=dev, generator=g)
            outs = {s: torch.empty((m * d, W), dtype=torch.int32, device=dev) for s in "ab"}
            oe = torch.empty(m * d, dtype=torch.int32, device=dev)

            def mm(s):
                lib, c = side[s]
                rc = lib.pai_matmul_dev(c._h, ct.data_ptr(), ex.data_ptr(), m, K, N.PAI_F64, x.data_ptr(), d,
                                        outs[s].data_ptr(), oe.data_ptr(), stream.cuda_stream)
                assert rc == 0, lib.pai_last_error()
            ab("pai_matmul_dev (1, 4096, 64), 2048 bits", {s: (lambda s=s: mm(s)) for s in "ab"}, outs)
        # side a alone: one level around k_modinv
        ct4, o4 = residues(4), torch.empty((4, W), dtype=torch.int32, device=dev)
        s4 = torch.zeros(1, dtype=torch.int32, device=dev)
        ca = side["a"][1]

        def neg4():
            assert lib_a.pai_neg_dev(ca._h, ct4.data_ptr(), 4, o4.data_ptr(), s4.data_ptr(), stream.cuda_stream) == 0
        neg4()
        t = [timed(neg4) for _ in range(args.rounds)]
        v, b = ctypes.c_int(), ctypes.c_int()
        assert lib_a.pai_debug_modinv_info(W, ctypes.byref(v), ctypes.byref(b)) == 0
        result["k_modinv"][str(nb)] = {"words": W, "vgprs_per_lane": v.value, "blocks_per_cu": b.value,
                                       "neg_dev_4_values_ms": {"median": round(statistics.median(t), 3),
                                                               "spread": round(max(t) - min(t), 3)}}
        del side, ca
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result["k_modinv"]), flush=True)


if __name__ == "__main__":
    main()
