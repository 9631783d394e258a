#!/usr/bin/env python3
"""A/B of the histogram over C ciphertext columns, in one process on one GPU, public-key context of the product library:
a = ONE pai_histogram_cols_dev over ct [N][C][W],
b = what a caller had before it: per column, pai_take_dev of the strided column into a contiguous buffer and
    pai_histogram_dev on it (C takes, C histograms, the index of every take built beforehand).
N = 262144 samples, F = 16 features, B = 32 bins (uniform ids, one node), C = 2 and 8, random residues mod n^2 with
exponent 0. One warm-up call per side, then --rounds rounds that alternate the sides; every call is timed by HIP events
on the null stream ("ms") and by the wall clock up to the end of the stream's work ("wall_ms"). Column c of a is asserted
identical to b's c-th result. Writes medians, spread (min, max) and the ratio to profiles/hist_cols_ab.json (--out).

    python tools/hist_cols_ab.py [--rounds 3] [--bits 1024,2048] [--quick] [--out profiles/hist_cols_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="one small case: a smoke run of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_cols_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, F, B = (4096, 4, 8) if args.quick else (262144, 16, 32)
    cells = F * B
    result = {"a_kind": "pai_histogram_cols_dev", "b_kind": "C x (pai_take_dev of the column + pai_histogram_dev)",
              "N": n, "F": F, "B": B, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "cases": []}
    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0)
        W = ctx.ct_words
        for C in (2, 8):
            d_bins = torch.randint(0, B, (n, F), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(n + C))
            ct = torch.randint(0, 2 ** 31 - 1, (n * C, W), dtype=torch.int32, device=dev)
            ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
            ex = torch.zeros(n * C, dtype=torch.int32, device=dev)
            col, col_e = torch.empty((n, W), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            out_a, oe_a = torch.empty((cells * C, W), dtype=torch.int32, device=dev), torch.empty(cells * C, dtype=torch.int32, device=dev)
            out_b, oe_b = torch.empty((C, cells, W), dtype=torch.int32, device=dev), torch.empty((C, cells), dtype=torch.int32, device=dev)
            d_cnt = torch.empty(cells, dtype=torch.int64, device=dev)
            index = [np.arange(n, dtype=np.int64) * C + c for c in range(C)]
            common = (N.PAI_BIN_U8, d_bins.data_ptr(), F, F, None, 1, B)

            def chk(rc):
                assert rc == 0, ctx.lib.pai_last_error()

            def run(s):
                if s == "a":
                    chk(ctx.lib.pai_histogram_cols_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n, C, *common, out_a.data_ptr(),
                                                       oe_a.data_ptr(), d_cnt.data_ptr(), None))
                    return
                for c in range(C):
                    chk(ctx.lib.pai_take_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n * C, index[c].ctypes.data, n,
                                             col.data_ptr(), col_e.data_ptr(), None))
                    chk(ctx.lib.pai_histogram_dev(ctx.handle, col.data_ptr(), col_e.data_ptr(), n, *common, out_b[c].data_ptr(),
                                                  oe_b[c].data_ptr(), d_cnt.data_ptr(), None))

            def timed(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record(torch.cuda.default_stream(dev))
                run(s)
                e1.record(torch.cuda.default_stream(dev))
                e1.synchronize()
                return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

            for s in "ab":
                run(s)                                         # warm-up: buffers, code objects
            torch.cuda.synchronize()
            ms, wall = {"a": [], "b": []}, {"a": [], "b": []}
            for _ in range(args.rounds):
                for s in "ab":
                    ev, wl = timed(s)
                    ms[s].append(ev)
                    wall[s].append(wl)
            assert torch.equal(out_a.view(cells, C, W).permute(1, 0, 2), out_b) and torch.equal(oe_a.view(cells, C).t(), oe_b), (nb, C)
            row = {"nb": nb, "C": C, "identical": True}
            for s in "ab":
                row[s] = {"ms": statistics.median(ms[s]), "ms_min": min(ms[s]), "ms_max": max(ms[s]),
                          "wall_ms": statistics.median(wall[s]), "wall_ms_min": min(wall[s]), "wall_ms_max": max(wall[s])}
            row["b_over_a_wall"] = row["b"]["wall_ms"] / row["a"]["wall_ms"]
            result["cases"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
