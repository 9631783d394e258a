#!/usr/bin/env python3
"""A/B of the encrypted histogram over a sparse bin matrix (pai_histogram_sparse_dev), in one process on one GPU,
public-key contexts:
a  = pai_histogram_sparse_dev of this library on the CSR matrix,
b  = pai_histogram_dev of a library built from the parent commit (--parent; this library's when the file is absent, the
     dense path is unchanged) on the DENSIFIED matrix: what a caller had to do before the sparse call existed.
Shapes: N = 262 144 samples, F = 256 one-hot columns, B = 2, default_bin 0, k stored entries (bin 1) per row for
k = 8, 32, 128, 256 (densities 1/32, 1/8, 1/2, 1); ciphertexts are random residues mod n^2 with exponent 0, so both sides
must give the same bits, which is asserted. One warm-up call per side, then --rounds rounds that alternate the sides,
every call timed by HIP events on the current stream. The density at which the two cross is interpolated (linearly in
log density) between the measured densities that bracket a ratio of 1.
One wide shape the dense call refuses (N F >= 2^31): 262 144 x 8 192 with 8 stored entries per row. Only the sparse side is
measured; the dense figure is the F = 256 time multiplied by 32, an EXTRAPOLATION linear in F, and marked as such.
Writes profiles/shist_ab.json (--out) after every case and prints each row.

    python tools/shist_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--bits 1024,2048] [--quick] [--out ...]
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_SAMPLES, F_AB, F_WIDE, B = 262144, 256, 8192, 2
STORED = (8, 32, 128, 256)


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def load_parent(path, ref, names):
    """A library of the parent commit: the entry points it has, declared as the current library declares them (it lacks the
    sparse call, so _native.load_library would refuse it)."""
    plib = ctypes.CDLL(path)
    for name in names:
        try:
            f = getattr(plib, name)
        except AttributeError:
            continue
        f.argtypes, f.restype = getattr(ref, name).argtypes, getattr(ref, name).restype
    return plib


def one_hot_rows(n, F, k, seed):
    """CSR arrays of n rows with k stored entries each, bin 1: row i holds the columns s_i + j F / k, s_i uniform."""
    stride = F // k
    start = np.random.default_rng(seed).integers(0, stride, n).astype(np.int32)
    indices = (start[:, None] + (np.arange(k, dtype=np.int32) * stride)[None, :]).reshape(-1)
    return np.arange(n + 1, dtype=np.int64) * k, indices, np.ones(n * k, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="4096 samples: a smoke run of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shist_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library(N.LIB_PATH)
    have_parent = os.path.exists(args.parent)
    plib = load_parent(args.parent, lib, N.EXPORTED) if have_parent else lib
    n = 4096 if args.quick else N_SAMPLES
    result = {"a_kind": "pai_histogram_sparse_dev, this library, CSR matrix",
              "b_kind": "pai_histogram_dev on the densified matrix, " + ("parent library" if have_parent else "this library"),
              "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "N": n, "B": B, "default_bin": 0,
              "sha256": {"library": sha256(N.LIB_PATH)}, "cases": [], "crossover": [], "wide": []}
    if have_parent:
        result["sha256"]["parent"] = sha256(args.parent)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")

    def stats(ms):
        med = statistics.median(ms)
        return {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=lib)
        pctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=plib) if have_parent else ctx
        W = ctx.ct_words
        g = torch.Generator(device=dev).manual_seed(nb + n)
        ct = torch.randint(0, 2 ** 31 - 1, (n, W), dtype=torch.int32, device=dev, generator=g)
        ct[:, W - 1] = 0                                       # < 2^(32 (W - 1)) < n^2
        ex = torch.zeros(n, dtype=torch.int32, device=dev)

        def sparse_side(F, csr, out):
            d_ptr, d_ind, d_dat = (torch.from_numpy(a).to(dev) for a in csr)
            d_def = torch.zeros(F, dtype=torch.int32, device=dev)

            def run():
                rc = lib.pai_histogram_sparse_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n, d_ptr.data_ptr(), d_ind.data_ptr(),
                                                  N.PAI_BIN_U8, d_dat.data_ptr(), F, d_def.data_ptr(), None, 1, B,
                                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream.cuda_stream)
                assert rc == 0, lib.pai_last_error()
            return run

        def outputs(F):
            return (torch.empty((F * B, W), dtype=torch.int32, device=dev), torch.empty(F * B, dtype=torch.int32, device=dev),
                    torch.empty(F * B, dtype=torch.int64, device=dev))

        dense_ms = {}
        rows = []
        for k in STORED:
            csr = one_hot_rows(n, F_AB, k, nb + k)
            dense = np.zeros((n, F_AB), dtype=np.uint8)
            dense[np.repeat(np.arange(n), k), csr[1]] = 1
            d_bins = torch.from_numpy(dense).to(dev)
            oa, ob = outputs(F_AB), outputs(F_AB)
            run_a = sparse_side(F_AB, csr, oa)

            def run_b():
                rc = plib.pai_histogram_dev(pctx.handle, ct.data_ptr(), ex.data_ptr(), n, N.PAI_BIN_U8, d_bins.data_ptr(), F_AB,
                                            F_AB, None, 1, B, ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr(),
                                            stream.cuda_stream)
                assert rc == 0, plib.pai_last_error()
            run_a()                                            # warm-up: buffers, code objects
            run_b()
            stream.synchronize()
            ms = {"a": [], "b": []}
            for _ in range(args.rounds):
                ms["a"].append(timed(run_a))
                ms["b"].append(timed(run_b))
            identical = bool(all(torch.equal(x, y) for x, y in zip(oa, ob)))
            assert identical, (nb, k)
            row = {"nb": nb, "F": F_AB, "stored_per_row": k, "density": k / F_AB, "nnz": n * k, "pairs": n * F_AB,
                   "identical": identical, "a": stats(ms["a"]), "b": stats(ms["b"])}
            row["speedup_b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
            row["a_faster_beyond_spread"] = bool(max(ms["a"]) < min(ms["b"]))
            row["a_slower_beyond_spread"] = bool(min(ms["a"]) > max(ms["b"]))
            dense_ms[k] = row["b"]["median_ms"]
            rows.append(row)
            result["cases"].append(row)
            save()
            print(json.dumps(row), flush=True)
            del d_bins, dense, oa, ob
        # where the ratio passes 1, between the measured densities
        cross = {"nb": nb, "density": None, "note": "the sparse call is faster at every measured density"}
        if rows[0]["speedup_b_over_a"] <= 1:
            cross["note"] = "the sparse call is not faster at the lowest measured density"
        for lo, hi in zip(rows, rows[1:]):
            r0, r1 = math.log(lo["speedup_b_over_a"]), math.log(hi["speedup_b_over_a"])
            if r0 > 0 >= r1:
                t = r0 / (r0 - r1)
                d = math.exp(math.log(lo["density"]) + t * (math.log(hi["density"]) - math.log(lo["density"])))
                cross = {"nb": nb, "density": round(d, 4), "between": [lo["density"], hi["density"]],
                         "note": "interpolated linearly in log density between the two measured densities"}
                break
        result["crossover"].append(cross)
        # the wide shape
        Fw = 64 if args.quick else F_WIDE
        csr = one_hot_rows(n, Fw, 8, nb + 7)
        ow = outputs(Fw)
        run_w = sparse_side(Fw, csr, ow)
        run_w()
        stream.synchronize()
        msw = [timed(run_w) for _ in range(args.rounds)]
        assert int(ow[2].sum().item()) == n * Fw
        base = statistics.median(dense_ms.values())
        wide = {"nb": nb, "F": Fw, "stored_per_row": 8, "nnz": n * 8, "pairs": n * Fw, "dense_call": "refused (N F >= 2^31)"
                if n * Fw >= 1 << 31 else "not run", "a": stats(msw),
                "b_extrapolated_ms": round(base * Fw / F_AB, 1), "b_is_extrapolated": True,
                "extrapolation": f"median dense time at F = {F_AB} ({round(base, 3)} ms) x {Fw // F_AB}, linear in F; not measured"}
        wide["speedup_extrapolated"] = round(wide["b_extrapolated_ms"] / wide["a"]["median_ms"], 1)
        result["wide"].append(wide)
        save()
        print(json.dumps(cross), flush=True)
        print(json.dumps(wide), flush=True)
        del ct, ex, ow, ctx, pctx
    save()


if __name__ == "__main__":
    main()
