#!/usr/bin/env python3
"""A/B of the segmented weighted sum (pai_segment_dot_dev), in one process on one GPU:
a = the test build under $FLEXPAI_SD_ALWAYS=1: every call through the fused kernels (kernels_sd.hpp; the same object
    code as the product's),
b = the composition that existed before the call: a device gather of ct[index] (torch.index_select), pai_mul_dev over
    the gathered entries and pai_segment_add_dev over consecutive ranges,
t = pai_segment_dot_dev with PAI_OPT_SEGDOT_FUSED = 0 (the call's own term path), for information.
Cases (nb, distinct, nnz, seglen): nnz entries drawn uniformly from `distinct` ciphertexts (reuse = nnz / distinct) in
segments of seglen; "csc_dense" is the dense 4096 x 64 feature block as CSC (every column lists all 4096 rows) and
"csc_2pct" the 4096 x 4096 block at 2 % density, for which the densified pai_matmul_dev is timed once as well
("matmul_dense_ms", --no-dense skips it). Ciphertexts are random units mod n^2 with exponents 12..14, scalars float64
standard normal (mixed signs). One warm-up call per side, then --rounds rounds that alternate the sides; every call is
timed by HIP events on the current stream; "default_path" is the path the product library's dispatch takes for the
case (1 = term path, 2 = fused). Writes the times, their spread, the ratios and whether a and b are
bit-identical to profiles/segdot_ab.json (--out) after every case, and prints each row.

    python tools/segdot_ab.py [--rounds 3] [--bits 1024,2048] [--quick] [--no-dense] [--out profiles/segdot_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (name, distinct, nnz, seglen)
SWEEP = [("reuse1", 65536, 65536, 64), ("reuse4", 16384, 65536, 64), ("reuse16", 4096, 65536, 64),
         ("reuse64", 1024, 65536, 64), ("len4", 4096, 65536, 4), ("len16", 4096, 65536, 16),
         ("len256", 4096, 65536, 256), ("len4096", 4096, 65536, 4096), ("nnz4k", 256, 4096, 64),
         ("nnz16k", 1024, 16384, 64), ("nnz128k", 4096, 131072, 64), ("nnz256k", 4096, 262144, 64),
         ("nnz512k", 4096, 524288, 64), ("nnz1m", 4096, 1048576, 64), ("nnz256k_reuse4", 65536, 262144, 64),
         ("nnz256k_reuse16", 16384, 262144, 64)]
QUICK = [("reuse16", 256, 4096, 64), ("len4", 256, 4096, 4)]


def cases(quick):
    for name, U, nnz, L in (QUICK if quick else SWEEP):
        rng = np.random.default_rng(U + nnz + L)
        idx = rng.integers(0, U, nnz).astype(np.int64)
        off = np.arange(0, nnz + 1, L, dtype=np.int64)
        if off[-1] != nnz:
            off = np.append(off, nnz)
        yield name, U, idx, off, None
    if quick:
        return
    K, d = 4096, 64
    yield "csc_dense", K, np.tile(np.arange(K, dtype=np.int64), d), np.arange(0, K * d + 1, K, dtype=np.int64), None
    d = 4096
    rng = np.random.default_rng(2)
    mask = rng.random((d, K)) < 0.02                          # [column][row]
    idx = np.nonzero(mask)[1].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    yield "csc_2pct", K, idx, off, np.nonzero(mask)[0].astype(np.int64)   # the entries' columns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="two small cases: a smoke run of the tool")
    ap.add_argument("--no-dense", action="store_true", help="skip the densified pai_matmul_dev of csc_2pct")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segdot_ab.json"))
    args = ap.parse_args()
    os.environ["FLEXPAI_SD_ALWAYS"] = "1"
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library(N.XCHECK_LIB_PATH)
    plib = N.load_library(N.LIB_PATH)                          # the product library: which path its dispatch takes
    result = {"a_kind": "test build, every call fused", "b_kind": "index_select + pai_mul_dev + pai_segment_add_dev",
              "t_kind": "pai_segment_dot_dev, PAI_OPT_SEGDOT_FUSED = 0", "rounds": args.rounds,
              "device": torch.cuda.get_device_name(dev), "cases": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")

    for nb in (int(v) for v in args.bits.split(",")):
        n = int(keys[str(nb)]["n"], 16)
        ctx = N.Context(n, 0, lib=lib)
        pctx = N.Context(n, 0, lib=plib)
        W = ctx.ct_words
        for name, U, idx, off, cols in cases(args.quick):
            nnz, nseg = idx.size, off.size - 1
            g = torch.Generator(device=dev).manual_seed(nb + nnz)
            ct = torch.randint(0, 2 ** 31 - 1, (U, W), dtype=torch.int32, device=dev, generator=g)
            ct[:, W - 1] = 0                                   # < 2^(32 (W - 1)) < n^2
            ex = torch.randint(12, 15, (U,), dtype=torch.int32, device=dev, generator=g)
            x = torch.randn(nnz, dtype=torch.float64, device=dev, generator=g)
            d_idx = torch.from_numpy(idx).to(dev)
            iota = np.arange(nnz, dtype=np.int64)
            outs = {s: (torch.empty((nseg, W), dtype=torch.int32, device=dev),
                        torch.empty(nseg, dtype=torch.int32, device=dev)) for s in "abt"}
            terms = (torch.empty((nnz, W), dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev))

            def chk(rc):
                assert rc == 0, lib.pai_last_error()

            def run(s):
                o, oe = outs[s]
                if s == "b":
                    gc, ge = ct.index_select(0, d_idx), ex.index_select(0, d_idx)
                    chk(lib.pai_mul_dev(ctx.handle, gc.data_ptr(), ge.data_ptr(), nnz, N.PAI_F64, x.data_ptr(), 1,
                                        terms[0].data_ptr(), terms[1].data_ptr(), None, stream.cuda_stream))
                    chk(lib.pai_segment_add_dev(ctx.handle, terms[0].data_ptr(), terms[1].data_ptr(), nnz, iota.ctypes.data,
                                                off.ctypes.data, nseg, o.data_ptr(), oe.data_ptr(), stream.cuda_stream))
                    return
                ctx.set_segdot_fused(s == "a")
                chk(lib.pai_segment_dot_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), U, idx.ctypes.data, off.ctypes.data,
                                            nseg, N.PAI_F64, x.data_ptr(), o.data_ptr(), oe.data_ptr(), None,
                                            stream.cuda_stream))
                assert ctx.segdot_path == (2 if s == "a" else 1)

            def timed(fn, *a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(*a)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for s in "abt":
                run(s)                                         # warm-up: buffers, code objects
            ms = {s: [] for s in "abt"}
            for _ in range(args.rounds):
                for s in "abt":
                    ms[s].append(timed(run, s))
            row = {"nb": nb, "case": name, "distinct": U, "nnz": int(nnz), "nseg": int(nseg),
                   "reuse": round(nnz / U, 2), "chunks": int(sum(-(-int(v) // 16) for v in np.diff(off))),
                   "identical": bool(all(torch.equal(outs["a"][i], outs[s][i]) for s in "bt" for i in (0, 1)))}
            chk(plib.pai_segment_dot_dev(pctx.handle, ct.data_ptr(), ex.data_ptr(), U, idx.ctypes.data, off.ctypes.data,
                                         nseg, N.PAI_F64, x.data_ptr(), outs["t"][0].data_ptr(), outs["t"][1].data_ptr(),
                                         None, stream.cuda_stream))
            row["default_path"] = pctx.segdot_path
            for s in "abt":
                med = statistics.median(ms[s])
                row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                          "spread": round((max(ms[s]) - min(ms[s])) / med, 4)}
            row["speedup_b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
            row["a_faster_beyond_spread"] = bool(min(ms["b"]) > max(ms["a"]))
            row["a_slower_beyond_spread"] = bool(min(ms["a"]) > max(ms["b"]))
            if cols is not None and not args.no_dense:
                K = d = U
                dense_h = np.zeros((K, d))
                dense_h[idx, cols] = x.cpu().numpy()
                dense = torch.from_numpy(dense_h).to(dev)
                mo = (torch.empty((d, W), dtype=torch.int32, device=dev), torch.empty(d, dtype=torch.int32, device=dev))

                def mm():
                    chk(lib.pai_matmul_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), 1, K, N.PAI_F64, dense.data_ptr(), d,
                                           mo[0].data_ptr(), mo[1].data_ptr(), stream.cuda_stream))

                row["matmul_dense_ms"] = round(timed(mm), 3)   # one call, no warm-up beyond the sides above
                row["matmul_path"] = ctx.matmul_path
                row["matmul_over_a"] = round(row["matmul_dense_ms"] / row["a"]["median_ms"], 2)
            result["cases"].append(row)
            save()
            print(json.dumps(row), flush=True)
            del ct, ex, x, outs, terms
        del ctx, pctx
    save()


if __name__ == "__main__":
    main()
