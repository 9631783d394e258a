#!/usr/bin/env python3
"""A/B of the encrypted-by-plain matrix product (pai_matmul_dev), in one process on one GPU:
a = this tree's library on its default path (the fused multi-exponentiation, kernels_mm.hpp),
b = a library built from the parent commit (--parent: the term path, k_mul + batch inversion + k_add over all terms;
    without one, this tree's library with PAI_OPT_MATMUL_FUSED = 0, which runs that code unchanged -- recorded as
    "b_kind").
Shapes (m, K, d): the he_otp_lr product enc_diff_y.dot(features) at a batch of 4096 with 64 features and with one, at
1024 and 2048 bits, and one 4096-bit shape. Ciphertexts are random units mod n^2 with exponents 12..14 (float32 values
of order 1), scalars float64 standard normal (14 windows, mixed signs). One warm-up call per side, then --rounds
rounds that alternate a and b; every call is timed by HIP events around pai_matmul_dev on the current stream. Writes the
times, their spread, the ratio, whether the outputs are identical and the product-count model's ratio
(tools/mm_model.py) to profiles/mm_ab.json (--out), and prints the same JSON.

    python tools/mm_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--shapes nb,m,K,d;...] [--always]
                          [--out profiles/mm_ab.json]

--always runs side a on the test build under $FLEXPAI_MM_ALWAYS=1, i.e. through the fused kernels whatever the shape
(the same object code as the product's): that is how the dispatch's class (flexpai.hip mm_take_fused) was measured
(profiles/mm_ab.json, profiles/mm_ab_sweep.json). Without it side a is the product library with its dispatch
(profiles/mm_ab_default.json: "a_path" 1 = the call stayed on the term path)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import mm_model  # noqa: E402

SHAPES = [(1024, 1, 4096, 64), (1024, 1, 4096, 1), (2048, 1, 4096, 64), (2048, 1, 4096, 1), (4096, 1, 1024, 16)]


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="", help="nb,m,K,d;nb,m,K,d;... instead of the default shapes")
    ap.add_argument("--always", action="store_true", help="side a: the test build with FLEXPAI_MM_ALWAYS=1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    if args.always:
        os.environ["FLEXPAI_MM_ALWAYS"] = "1"
    path_a = N.XCHECK_LIB_PATH if args.always else N.LIB_PATH
    lib_a = N.load_library(path_a)
    have_parent = os.path.exists(args.parent)
    lib_b = N.load_library(args.parent) if have_parent else lib_a
    result = {"b_kind": "parent library" if have_parent else "same library, PAI_OPT_MATMUL_FUSED = 0",
              "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "shapes": []}
    shapes = [tuple(int(v) for v in t.split(",")) for t in args.shapes.split(";") if t] or SHAPES
    result["a_kind"] = "test build, every call fused" if args.always else "product library, default dispatch"
    for nb, m, K, d in shapes:
        n = int(keys[str(nb)]["n"], 16)
        ca = N.Context(n, 0, lib=lib_a)
        cb = N.Context(n, 0, lib=lib_b)
        if not have_parent:
            cb.set_matmul_fused(False)
        W = ca.ct_words
        g = torch.Generator(device=dev).manual_seed(nb + d)
        ct = torch.randint(0, 2 ** 31 - 1, (m * K, W), dtype=torch.int32, device=dev, generator=g)
        ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
        ex = torch.randint(12, 15, (m * K,), dtype=torch.int32, device=dev, generator=g)
        x = torch.randn((K, d), dtype=torch.float64, device=dev, generator=g)
        outs = {s: (torch.empty((m * d, W), dtype=torch.int32, device=dev), torch.empty(m * d, dtype=torch.int32, device=dev))
                for s in "ab"}
        side = {"a": (lib_a, ca), "b": (lib_b, cb)}

        def call(s):
            lib, c = side[s]
            o, oe = outs[s]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = lib.pai_matmul_dev(c.handle, ct.data_ptr(), ex.data_ptr(), m, K, N.PAI_F64, x.data_ptr(), d,
                                    o.data_ptr(), oe.data_ptr(), stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for s in "ab":
            call(s)                                        # warm-up: buffers, code objects
        ms = {"a": [], "b": []}
        for _ in range(args.rounds):
            for s in "ab":
                ms[s].append(call(s))
        neg = float((x < 0).any(dim=1).double().mean().item())
        row = {"nb": nb, "m": m, "K": K, "d": d, "neg_rows": round(neg, 3), "a_path": ca.matmul_path,
               "identical": bool(torch.equal(outs["a"][0], outs["b"][0]) and torch.equal(outs["a"][1], outs["b"][1]))}
        for s in "ab":
            med = statistics.median(ms[s])
            row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                      "spread": round((max(ms[s]) - min(ms[s])) / med, 4)}
        row["speedup_b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
        row["faster_beyond_spread"] = bool(min(ms["b"]) > max(ms["a"]))
        row["model_product_ratio"] = mm_model.counts(m, K, d, 14, neg)["ratio_term_over_fused"]
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del ca, cb
    result["sha256"] = {"a": sha256(path_a)}
    if have_parent:
        result["sha256"]["b"] = sha256(args.parent)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
