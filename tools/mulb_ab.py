#!/usr/bin/env python3
"""A/B of the broadcast multiply (pai_mul_bcast_dev), in one process on one GPU:
a = the comb (PAI_OPT_MUL_BCAST = 2: k_mulb_plan, k_mulb_tab, k_mulb_acc, kernels_mulb.hpp),
b = the term path of the same library (PAI_OPT_MUL_BCAST = 0: one k_mul chain per output, ciphertext stride 0 along
    the row -- the parent commit's chain without its replication),
r = pai_mul_dev over the ciphertexts replicated F times on the device beforehand (what `enc[:, None] * X` ran before
    this entry point, without its host-side replication and upload), on --parent's library when that file exists and on
    this tree's otherwise ("r_kind"); timed at the F of --replicated only.
Shapes (nb, N, F): N = 4096 at 1024 and 2048 bits, N = 512 at 4096 bits, F in 2, 4, 8, 16, 64, 256. Ciphertexts are
random units mod n^2, scalars float64 standard normal (14 windows, mixed signs: both sides close with the batch
inversion over all outputs). One warm-up call per side, then --rounds rounds that alternate the sides; every call is
timed by HIP events around the entry point on the current stream. Writes the times, their spread, the ratio and whether
the outputs are identical to profiles/mulb_ab.json (--out), and prints the same JSON.

    python tools/mulb_ab.py [--rounds 3] [--shapes nb,N,F;...] [--replicated 64] [--parent ab/libflexpai_parent.so]
                            [--out profiles/mulb_ab.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402

FS = (2, 4, 8, 16, 64, 256)
SHAPES = [(nb, N, F) for nb, N in ((1024, 4096), (2048, 4096), (4096, 512)) for F in FS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="", help="nb,N,F;nb,N,F;... instead of the default shapes")
    ap.add_argument("--replicated", type=int, default=64, help="the F at which side r is timed as well (0: never)")
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mulb_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library(N.LIB_PATH)
    have_parent = os.path.exists(args.parent)
    lib_r = N.load_library(args.parent) if have_parent else lib
    result = {"a_kind": "PAI_OPT_MUL_BCAST = 2 (comb)", "b_kind": "same library, PAI_OPT_MUL_BCAST = 0 (term path)",
              "r_kind": "pai_mul_dev over replicated ciphertexts, " + ("parent library" if have_parent else "same library"),
              "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "shapes": []}
    shapes = [tuple(int(v) for v in t.split(",")) for t in args.shapes.split(";") if t] or SHAPES
    for nb, rows, F in shapes:
        n = int(keys[str(nb)]["n"], 16)
        ctx = {"a": N.Context(n, 0, lib=lib), "b": N.Context(n, 0, lib=lib), "r": N.Context(n, 0, lib=lib_r)}
        ctx["a"].mul_bcast_mode, ctx["b"].mul_bcast_mode = 2, 0
        W, T = ctx["a"].ct_words, rows * F
        g = torch.Generator(device=dev).manual_seed(nb + F)
        ct = torch.randint(0, 2 ** 31 - 1, (rows, W), dtype=torch.int32, device=dev, generator=g)
        ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
        ex = torch.randint(12, 15, (rows,), dtype=torch.int32, device=dev, generator=g)
        x = torch.randn((rows, F), dtype=torch.float64, device=dev, generator=g)
        sides = "abr" if F == args.replicated else "ab"
        outs = {s: (torch.empty((T, W), dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
                    torch.empty(T, dtype=torch.int32, device=dev)) for s in sides}
        if "r" in sides:
            ct_r, ex_r = ct.repeat_interleave(F, dim=0).contiguous(), ex.repeat_interleave(F).contiguous()

        def call(s):
            o, oe, st = outs[s]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if s == "r":
                rc = lib_r.pai_mul_dev(ctx[s].handle, ct_r.data_ptr(), ex_r.data_ptr(), T, N.PAI_F64, x.data_ptr(), 1,
                                       o.data_ptr(), oe.data_ptr(), st.data_ptr(), stream.cuda_stream)
            else:
                rc = lib.pai_mul_bcast_dev(ctx[s].handle, ct.data_ptr(), ex.data_ptr(), rows, N.PAI_F64, x.data_ptr(), F,
                                           o.data_ptr(), oe.data_ptr(), st.data_ptr(), stream.cuda_stream)
            assert rc == 0, (lib_r if s == "r" else lib).pai_last_error()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for s in sides:
            call(s)                                        # warm-up: buffers, code objects
        ms = {s: [] for s in sides}
        for _ in range(args.rounds):
            for s in sides:
                ms[s].append(call(s))
        row = {"nb": nb, "N": rows, "F": F, "a_path": ctx["a"].mul_bcast_path, "b_path": ctx["b"].mul_bcast_path,
               "identical": all(bool(torch.equal(outs["a"][k], outs[s][k])) for s in sides for k in range(3))}
        for s in sides:
            med = statistics.median(ms[s])
            row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                      "spread": round((max(ms[s]) - min(ms[s])) / med, 4)}
        row["speedup_b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
        row["faster_beyond_spread"] = bool(min(ms["b"]) > max(ms["a"]))
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del ctx, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
