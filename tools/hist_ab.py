#!/usr/bin/env python3
"""A/B of the encrypted histogram (pai_histogram_dev), in one process on one GPU, public-key contexts:
a  = pai_histogram_dev of the product library: counts and member lists built on the device from the bin matrix, the
     shipped kernel over the runs, the segmented add over the runs' partials; and its variants on the test build (the
     same object code, selected through the environment): "acc64", "acc128", "acc256" = k_hist_acc over runs of that
     length, "rows" = k_add over device-built gather rows (runs of 64),
b  = the route that existed before the call: the caller builds the index lists in Python (a stable argsort of
     node * B + bin per feature, slices concatenated in cell order) and calls pai_segment_add_dev; "b" times the list
     building and the call, "b_call" the call alone over lists built beforehand.
Cases (N samples, F features, B bins, nodes): bin ids uniform in [0, B), node ids uniform in [0, nodes). Ciphertexts are
random residues mod n^2 with exponent 0 (labels, as IV_FFS encrypts them). One warm-up call per side, then --rounds
rounds that alternate the sides; every call is timed by HIP events on the current stream ("ms") and by the wall clock
around the call and a stream synchronisation ("wall_ms": the host work of b's list building is outside the events). The
outputs of a and b are asserted identical. Writes the times, their spread and the ratios to profiles/hist_ab.json (--out)
after every case, and prints each row. The acceptance line is a's wall time against b's, list building included.

    python tools/hist_ab.py [--rounds 3] [--bits 1024,2048] [--quick] [--out profiles/hist_ab.json]
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

# (name, N, F, B, nodes)
SHAPES = [("n256k_f16_b32", 262144, 16, 32, 1), ("n256k_f16_b32_nodes8", 262144, 16, 32, 8), ("n16k_f64_b16", 16384, 64, 16, 1)]
QUICK = [("quick", 4096, 4, 8, 2)]


def build_lists(bins, B, node, nodes):
    """(index, seg_off) of the cells in the order (node, feature, bin): what a caller of pai_segment_add builds."""
    N, F = bins.shape
    v = np.zeros(N, dtype=np.int64) if node is None else node.astype(np.int64)
    pieces = [[None] * F for _ in range(nodes)]
    sizes = np.zeros((nodes, F, B), dtype=np.int64)
    for f in range(F):
        key = v * B + bins[:, f]
        order = np.argsort(key, kind="stable")
        cnt = np.bincount(key, minlength=nodes * B)
        cs = np.concatenate([[0], np.cumsum(cnt)])
        for w in range(nodes):
            pieces[w][f] = order[cs[w * B]:cs[(w + 1) * B]]
        sizes[:, f, :] = cnt.reshape(nodes, B)
    idx = np.concatenate([p for row in pieces for p in row]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes.reshape(-1))]).astype(np.int64)
    return idx, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="one small case: a smoke run of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library(N.LIB_PATH)
    xlib = N.load_library(N.XCHECK_LIB_PATH)
    variants = {"acc64": {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "64"},
                "acc128": {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "128"},
                "acc256": {"FLEXPAI_HIST_ACC": "1", "FLEXPAI_HIST_RUN": "256"}, "rows": {"FLEXPAI_HIST_ACC": "0"}}
    result = {"a_kind": f"pai_histogram_dev, product library (runs of {N.HIST_RUN})",
              "variant_kinds": "test build: acc<R> = k_hist_acc over runs of R, rows = k_add over device-built gather rows",
              "b_kind": "Python list building (argsort per feature, concatenate) + pai_segment_add_dev",
              "b_call_kind": "pai_segment_add_dev alone, lists built beforehand", "rounds": args.rounds,
              "device": torch.cuda.get_device_name(dev), "cases": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")

    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=lib)
        xctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=xlib)
        W = ctx.ct_words
        for name, n, F, B, nodes in (QUICK if args.quick else SHAPES):
            rng = np.random.default_rng(n + F + B + nodes)
            bins = rng.integers(0, B, (n, F)).astype(np.uint8)
            node = None if nodes == 1 else rng.integers(0, nodes, n).astype(np.int32)
            cells = nodes * F * B
            g = torch.Generator(device=dev).manual_seed(nb + n)
            ct = torch.randint(0, 2 ** 31 - 1, (n, W), dtype=torch.int32, device=dev, generator=g)
            ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
            ex = torch.zeros(n, dtype=torch.int32, device=dev)
            d_bins = torch.from_numpy(bins).to(dev)
            d_node = None if node is None else torch.from_numpy(node).to(dev)
            outs = {s: (torch.empty((cells, W), dtype=torch.int32, device=dev),
                        torch.empty(cells, dtype=torch.int32, device=dev)) for s in ("a", "b", "b_call", *variants)}
            d_cnt = torch.empty(cells, dtype=torch.int64, device=dev)
            lists = build_lists(bins, B, node, nodes)

            def chk(rc):
                assert rc == 0, lib.pai_last_error()

            def run(s):
                o, oe = outs[s]
                if s == "a" or s in variants:
                    for k in ("FLEXPAI_HIST_ACC", "FLEXPAI_HIST_RUN"):
                        os.environ.pop(k, None)
                    os.environ.update(variants.get(s, {}))
                    l, cx = (lib, ctx) if s == "a" else (xlib, xctx)
                    chk(l.pai_histogram_dev(cx.handle, ct.data_ptr(), ex.data_ptr(), n, N.PAI_BIN_U8, d_bins.data_ptr(), F, F,
                                              None if d_node is None else d_node.data_ptr(), nodes, B, o.data_ptr(),
                                              oe.data_ptr(), d_cnt.data_ptr(), stream.cuda_stream))
                    return
                idx, off = build_lists(bins, B, node, nodes) if s == "b" else lists
                chk(lib.pai_segment_add_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n, idx.ctypes.data, off.ctypes.data,
                                            cells, o.data_ptr(), oe.data_ptr(), stream.cuda_stream))

            def timed(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                run(s)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

            sides = ("a", "b", "b_call", *variants)
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
            identical = bool(all(torch.equal(outs["a"][i], outs[s][i]) for s in sides[1:] for i in (0, 1)))
            assert identical, (nb, name)
            assert np.array_equal(d_cnt.cpu().numpy(), np.diff(lists[1])), (nb, name)
            row = {"nb": nb, "case": name, "N": n, "F": F, "B": B, "nodes": nodes, "entries": int(lists[0].size),
                   "cells": cells, "identical": identical}
            for s in sides:
                med, wmed = statistics.median(ms[s]), statistics.median(wall[s])
                row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                          "spread": round((max(ms[s]) - min(ms[s])) / med, 4),
                          "wall_ms": [round(v, 3) for v in wall[s]], "median_wall_ms": round(wmed, 3),
                          "wall_spread": round((max(wall[s]) - min(wall[s])) / wmed, 4)}
            row["speedup_b_over_a_wall"] = round(row["b"]["median_wall_ms"] / row["a"]["median_wall_ms"], 3)
            row["speedup_b_call_over_a_wall"] = round(row["b_call"]["median_wall_ms"] / row["a"]["median_wall_ms"], 3)
            for s in variants:
                row[f"speedup_{s}_over_a_wall"] = round(row["a"]["median_wall_ms"] / row[s]["median_wall_ms"], 3)
            row["a_slower_than_b_beyond_spread"] = bool(min(wall["a"]) > max(wall["b"]))
            row["a_faster_than_b_beyond_spread"] = bool(min(wall["b"]) > max(wall["a"]))
            result["cases"].append(row)
            save()
            print(json.dumps(row), flush=True)
            del ct, ex, outs
        del ctx, xctx
    save()


if __name__ == "__main__":
    main()
