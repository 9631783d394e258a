#!/usr/bin/env python3
"""A/B of the prefix sums of ciphertext arrays (pai_cumsum_dev), in one process on one GPU, public-key contexts:
a     = pai_cumsum_dev with the automatic tile length (PAI_OPT_SCAN_TILE = 0); "t<T>" = the same call with tiles of T
        forced (T >= L: the row chains), the sweep the automatic rule's floor is read from,
b     = what a caller of the library could do before the call existed:
        rows     L - 1 successive pai_add_dev calls (k = 2) over device-resident column arrays: the running sum and the
                 next column lie next to each other, and each call writes the next pair's first half. The columns are
                 gathered into that layout OUTSIDE the timed region, which favours b;
        vector   ceil(log2 L) shifted passes: pass d copies the vector shifted by d next to itself (the first d entries
                 become the identity: ciphertext 1, exponent INT32_MIN) and one pai_add_dev (k = 2) adds the two.
Shapes (outer, L, inner): (8192, 32, 1) = 64 nodes x 128 features x 32 bins; (1024, 256, 1); (1, 32, 8192) = the same
cells scanned along a non-last axis; (1, 2^18, 1). Ciphertexts are random residues mod n^2 with exponent 0; the case
"hist_8192x32_mixed" gives every 16th row exponents drawn from 0 .. 3 (the others stay at 0), so that rows of one exponent
share their waves with rows that square, the lock-step cost the kernel leaves to its uniform rows. One warm-up
call per side, then --rounds rounds that alternate the sides; every call is timed by HIP events on the current stream
("ms") and by the wall clock around the call and a stream synchronisation ("wall_ms"). The outputs of all sides are
asserted identical. Writes the times, their spread and the ratios to profiles/cumsum_ab.json (--out) after every case,
and prints each row.

    python tools/cumsum_ab.py [--rounds 3] [--bits 1024,2048] [--quick] [--out profiles/cumsum_ab.json]
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

EMPTY = -(1 << 31)
# (name, outer, L, inner, forced tiles, every how many rows one has mixed exponents (0: none))
SHAPES = [("hist_8192x32", 8192, 32, 1, (4, 8, 16, 32), 0), ("rows_1024x256", 1024, 256, 1, (4, 8, 16, 32, 64, 256), 0),
          ("axis0_32x8192", 1, 32, 8192, (4, 8, 16, 32), 0),
          ("vector_2p18", 1, 1 << 18, 1, (4, 8, 16, 32, 64, 128, 256, 1024), 0),
          ("hist_8192x32_mixed", 8192, 32, 1, (8, 32), 16)]
QUICK = [("quick_rows", 64, 8, 1, (4, 8), 0), ("quick_vector", 1, 1000, 1, (16, 64), 0), ("quick_mixed", 64, 8, 1, (4, 8), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="two small cases: a smoke run of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cumsum_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library(N.LIB_PATH)
    result = {"a_kind": "pai_cumsum_dev, automatic tile length", "t_kind": "pai_cumsum_dev with PAI_OPT_SCAN_TILE = T",
              "b_kind": "rows: L - 1 pai_add_dev calls (k = 2) over pre-gathered columns; vector: ceil(log2 L) shifted "
                        "copies + pai_add_dev passes",
              "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "cases": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")

    def chk(rc):
        assert rc == 0, lib.pai_last_error()

    mismatches = []
    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=lib)
        W = ctx.ct_words
        for name, outer, L, inner, tiles, mixed in (QUICK if args.quick else SHAPES):
            n = outer * L * inner
            rows = outer * inner
            g = torch.Generator(device=dev).manual_seed(nb + n)
            ct = torch.randint(0, 2 ** 31 - 1, (outer, L, inner, W), dtype=torch.int32, device=dev, generator=g)
            ct[..., W - 1] = 0                                 # < 2^(32 (W - 1)) < n^2
            ex = torch.zeros((outer, L, inner), dtype=torch.int32, device=dev)
            if mixed:
                ex[::mixed] = torch.randint(0, 4, ex[::mixed].shape, dtype=torch.int32, device=dev, generator=g)
            sides = ["a"] + [f"t{t}" for t in tiles] + ["b"]
            out = {s: (torch.empty((outer, L, inner, W), dtype=torch.int32, device=dev),
                       torch.empty(n, dtype=torch.int32, device=dev)) for s in sides if s != "b"}
            paths = {}
            vector = rows == 1
            if vector:
                # b: X[0] the vector, X[1] its shifted copy; the passes alternate between X and Y
                X = torch.empty((2, L, W), dtype=torch.int32, device=dev)
                Y = torch.empty((2, L, W), dtype=torch.int32, device=dev)
                XE = torch.empty((2, L), dtype=torch.int32, device=dev)
                YE = torch.empty((2, L), dtype=torch.int32, device=dev)
                one = torch.zeros(W, dtype=torch.int32, device=dev)
                one[0] = 1
            else:
                # b: Z[2 j] = the running sum up to column j - 1, Z[2 j + 1] = column j; pair j writes Z[2 (j + 1)]
                Z = torch.empty((2 * L + 1, rows, W), dtype=torch.int32, device=dev)
                ZE = torch.zeros((2 * L + 1, rows), dtype=torch.int32, device=dev)
                cols = ct.permute(1, 0, 2, 3).reshape(L, rows, W)
                Z[1::2][:L] = cols                             # the gather, outside the timed region
                Z[2] = cols[0]
                ecols = ex.permute(1, 0, 2).reshape(L, rows)
                ZE[1::2][:L] = ecols
                ZE[2] = ecols[0]

            def run(s):
                if s != "b":
                    ctx.set_scan_tile(0 if s == "a" else int(s[1:]))
                    o, oe = out[s]
                    chk(lib.pai_cumsum_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), outer, L, inner, 0, o.data_ptr(),
                                           oe.data_ptr(), stream.cuda_stream))
                    paths[s] = ctx.scan_path
                    return
                if vector:
                    src, se, dst, de = X, XE, Y, YE
                    src[0].copy_(ct.view(L, W))
                    se[0].copy_(ex.view(L))
                    d = 1
                    while d < L:
                        src[1, d:].copy_(src[0, :L - d])
                        src[1, :d] = one
                        se[1, d:].copy_(se[0, :L - d])
                        se[1, :d] = EMPTY
                        chk(lib.pai_add_dev(ctx.handle, src.data_ptr(), se.data_ptr(), 2, L, dst.data_ptr(), de.data_ptr(),
                                            stream.cuda_stream))
                        src, se, dst, de = dst, de, src, se
                        d *= 2
                    run.b_out, run.b_exp = src[0], se[0]
                    return
                for j in range(1, L):
                    chk(lib.pai_add_dev(ctx.handle, Z[2 * j].data_ptr(), ZE[2 * j].data_ptr(), 2, rows, Z[2 * j + 2].data_ptr(),
                                        ZE[2 * j + 2].data_ptr(), stream.cuda_stream))

            def b_result():
                if vector:
                    return run.b_out.view(outer, L, inner, W), run.b_exp.reshape(-1)
                return (Z[2::2][:L].reshape(L, outer, inner, W).permute(1, 0, 2, 3),
                        ZE[2::2][:L].reshape(L, outer, inner).permute(1, 0, 2).reshape(-1))

            def timed(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                run(s)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

            for s in sides:
                run(s)                                         # warm-up: buffers, code objects
            stream.synchronize()
            ms = {s: [] for s in sides}
            wall = {s: [] for s in sides}
            for _ in range(args.rounds):
                for s in sides:
                    ev, wl = timed(s)
                    ms[s].append(ev)
                    wall[s].append(wl)
            ctx.set_scan_tile(0)
            identical = bool(all(torch.equal(out["a"][i], out[s][i]) for s in sides[1:-1] for i in (0, 1))
                             and torch.equal(out["a"][0], b_result()[0]) and torch.equal(out["a"][1], b_result()[1]))
            if not identical:
                mismatches.append((nb, name))
            row = {"nb": nb, "case": name, "outer": outer, "L": L, "inner": inner, "mixed_every": mixed, "identical": identical,
                   "paths": {s: paths[s] for s in sides if s != "b"}}
            for s in sides:
                med, wmed = statistics.median(ms[s]), statistics.median(wall[s])
                row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                          "spread": round((max(ms[s]) - min(ms[s])) / med, 4),
                          "wall_ms": [round(v, 3) for v in wall[s]], "median_wall_ms": round(wmed, 3),
                          "wall_spread": round((max(wall[s]) - min(wall[s])) / wmed, 4)}
            row["speedup_b_over_a_wall"] = round(row["b"]["median_wall_ms"] / row["a"]["median_wall_ms"], 3)
            row["a_slower_than_b_beyond_spread"] = bool(min(wall["a"]) > max(wall["b"]))
            row["a_faster_than_b_beyond_spread"] = bool(min(wall["b"]) > max(wall["a"]))
            best = min((s for s in sides if s != "b"), key=lambda s: row[s]["median_wall_ms"])
            row["fastest_side"] = best
            result["cases"].append(row)
            save()
            print(json.dumps({k: (v if not isinstance(v, dict) or k == "paths" else v["median_wall_ms"]) for k, v in row.items()}),
                  flush=True)
            del ct, ex, out
            if vector:
                del X, Y, XE, YE
            else:
                del Z, ZE, cols, ecols
            torch.cuda.empty_cache()
        ctx.close()
    save()
    assert not mismatches, f"outputs differ: {mismatches}"


if __name__ == "__main__":
    main()
