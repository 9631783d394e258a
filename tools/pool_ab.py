#!/usr/bin/env python3
"""A/B of the obfuscator pool (include/flexpai.h "Obfuscator pool", csrc/kernels_pool.hpp), one process, one GPU,
device-resident buffers, HIP events on the current stream, one warm-up per side and then --rounds interleaved rounds.

(a) fused against composed: pai_encrypt_dev(PAI_OBF_POOL) with PAI_OPT_POOL_FUSED 1 (k_pool_enc) against 0 (k_pool_join,
    the PAI_OBF_NONE encryption, k_obf_mul) on public-key-only contexts: 2^20 float32 elements at 1024 and 2048 bits, 2^18
    at 4096. The ring is refilled by pai_pool_put_dev outside the timed window. Outputs must be identical. The fused
    call is one kernel, so its time is also set against the bytes it moves (one row in, one ciphertext, exponent and
    status out, the plaintext in) at the HBM rate.
(b) pooled encryption against the warm PAI_OBF_RNG call of the same party: a 2048-bit key holder (fixed-base tables
    resident), a 2048-bit public-key-only context (public tables resident), 1 000 and 2^20 elements each, and a 4096-bit
    public-key-only context, 1 000 and 2^18. The RNG side runs on a library built from the parent commit when --parent
    exists (this change touches none of its kernels), else on this library.
(c) fill cost: pai_pool_fill_dev of 2^20 entries (2^18 at 4096 bits) against pai_encrypt_dev of as many int64 zeros on the
    same route; the difference is k_pool_split.

    python tools/pool_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--parts abc] [--small] [--out profiles/pool_ab.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402

RK = bytes(range(32))
HBM_BYTES_PER_S = 8.0e12          # MI355X peak


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def load_parent(path, ref, names):
    """A library of the parent commit: the entry points it has, declared as the current library declares them (it lacks the
    pool's, so _native.load_library would refuse it)."""
    plib = ctypes.CDLL(path)
    for name in names:
        try:
            f = getattr(plib, name)
        except AttributeError:
            continue
        f.argtypes, f.restype = getattr(ref, name).argtypes, getattr(ref, name).restype
    return plib


def stats(ms, size):
    med = statistics.median(ms)
    return {"ms": [round(v, 4) for v in ms], "median_ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "elems_per_s": round(size / med * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--small", action="store_true", help="2^12 elements instead of 2^20 / 2^18: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library()
    have_parent = os.path.exists(args.parent)
    plib = load_parent(args.parent, lib, N.EXPORTED) if have_parent else lib
    big = {1024: 1 << 20, 2048: 1 << 20, 4096: 1 << 18}
    if args.small:
        big = {nb: 1 << 12 for nb in big}
    result = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "small": args.small,
              "sha256": {"library": sha256(N.LIB_PATH)}, "rng_side": "parent library" if have_parent else "this library"}
    if have_parent:
        result["sha256"]["parent"] = sha256(args.parent)

    def key(nb):
        k = keys[str(nb)]
        return int(k["n"], 16), int(k["p"], 16), int(k["q"], 16)

    def chk(rc, which=lib):
        assert rc == 0, which.pai_last_error().decode()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    class Bufs:
        """Device buffers of one (context, size): float32 plaintexts, random rho below n^2, outputs."""

        def __init__(self, ctx, size):
            W = ctx.ct_words
            g = torch.Generator(device=dev).manual_seed(size + W)
            self.size, self.W = size, W
            self.x = torch.randn(size, dtype=torch.float32, device=dev, generator=g)
            self.rho = torch.randint(0, 2 ** 31 - 1, (size, W), dtype=torch.int32, device=dev, generator=g)
            self.rho[:, W - 1] = 0                     # < 2^(32 (W - 1)) < n^2
            self.zeros = torch.zeros(size, dtype=torch.int64, device=dev)
            self.ct = torch.empty((size, W), dtype=torch.int32, device=dev)
            self.exp = torch.empty(size, dtype=torch.int32, device=dev)
            self.st = torch.empty(size, dtype=torch.int32, device=dev)

    def refill(ctx, b):
        chk(lib.pai_pool_put_dev(ctx.handle, b.rho.data_ptr(), b.size, stream.cuda_stream))

    def pooled(ctx, b, out=None):
        out = b.ct if out is None else out
        chk(lib.pai_encrypt_dev(ctx.handle, N.PAI_F32, b.x.data_ptr(), b.size, N.PAI_EXP_AUTO, 0, N.PAI_OBF_POOL, None, 0, 0,
                                None, 0, out.data_ptr(), b.exp.data_ptr(), b.st.data_ptr(), stream.cuda_stream))

    def rng_call(ctx, b, x=None, dtype=None):
        x = b.x if x is None else x
        chk(ctx.lib.pai_encrypt_dev(ctx.handle, N.PAI_F32 if dtype is None else dtype, x.data_ptr(), b.size, N.PAI_EXP_AUTO, 0,
                                    N.PAI_OBF_RNG, None, 0, 0, RK, 0, b.ct.data_ptr(), b.exp.data_ptr(), b.st.data_ptr(),
                                    stream.cuda_stream), ctx.lib)

    # ------------------------------------------------------------ (a) fused against composed
    if "a" in args.parts:
        rows = []
        for nb in (1024, 2048, 4096):
            n, _, _ = key(nb)
            ctx = N.Context(n, 0)
            size = big[nb]
            b = Bufs(ctx, size)
            ctx.pool_reserve(size)
            outs = {}
            ms = {"fused": [], "composed": []}
            for rnd in range(args.rounds + 1):          # round 0: the warm-up and the identity check
                for side in ("fused", "composed"):
                    ctx.set_pool_fused(side == "fused")
                    refill(ctx, b)
                    torch.cuda.synchronize()
                    if rnd == 0:
                        outs[side] = torch.empty_like(b.ct)
                        pooled(ctx, b, outs[side])
                        torch.cuda.synchronize()
                    else:
                        ms[side].append(timed(lambda: pooled(ctx, b)))
            row = {"nb": nb, "size": size, "identical": bool(torch.equal(outs["fused"], outs["composed"])),
                   "fused": stats(ms["fused"], size), "composed": stats(ms["composed"], size)}
            row["composed_over_fused"] = round(row["composed"]["median_ms"] / row["fused"]["median_ms"], 3)
            row["fused_faster_beyond_spread"] = bool(max(ms["fused"]) < min(ms["composed"]))
            per_elem = 2 * ctx.pt_words * 4 + ctx.ct_words * 4 + 4 + 4 + 4   # row, ciphertext, plaintext, exponent, status
            row["bytes_per_element"] = per_elem
            row["fused_bytes_per_s"] = round(per_elem * size / row["fused"]["median_ms"] * 1e3)
            row["fused_share_of_hbm_peak"] = round(row["fused_bytes_per_s"] / HBM_BYTES_PER_S, 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del b, outs, ctx
            torch.cuda.empty_cache()
        result["a_fused_vs_composed"] = rows

    # ------------------------------------------------------------ parties of (b) and (c)
    def parties():
        n, p, q = key(2048)
        a = N.Context(n, 0, p, q)
        a.prepare_fixed_base()
        pa = N.Context(n, 0, p, q, lib=plib) if have_parent else a
        if have_parent:
            pa.prepare_fixed_base()
        yield "2048-bit key holder, fixed-base window %d" % a.fb_window, 2048, a, pa
        del a, pa
        torch.cuda.empty_cache()
        a = N.Context(n, 0)
        a.prepare_public_fixed_base()
        pa = N.Context(n, 0, lib=plib) if have_parent else a
        if have_parent:
            pa.prepare_public_fixed_base()
        yield "2048-bit public-key-only, public tables resident", 2048, a, pa
        del a, pa
        torch.cuda.empty_cache()
        n, _, _ = key(4096)
        a = N.Context(n, 0)
        yield "4096-bit public-key-only", 4096, a, (N.Context(n, 0, lib=plib) if have_parent else a)

    if "b" in args.parts or "c" in args.parts:
        rows_b, rows_c = [], []
        for name, nb, ctx, pctx in parties():
            for size in (1000, big[nb]):
                b = Bufs(ctx, size)
                ctx.pool_reserve(size)
                if "b" in args.parts:
                    ms = {"pooled": [], "rng": []}
                    for rnd in range(args.rounds + 1):
                        refill(ctx, b)
                        torch.cuda.synchronize()
                        t = timed(lambda: pooled(ctx, b))
                        u = timed(lambda: rng_call(pctx, b))
                        if rnd:
                            ms["pooled"].append(t)
                            ms["rng"].append(u)
                    row = {"party": name, "size": size, "pooled": stats(ms["pooled"], size), "rng": stats(ms["rng"], size)}
                    row["rng_over_pooled"] = round(row["rng"]["median_ms"] / row["pooled"]["median_ms"], 2)
                    row["pooled_faster_beyond_spread"] = bool(max(ms["pooled"]) < min(ms["rng"]))
                    rows_b.append(row)
                    print(json.dumps(row), flush=True)
                if "c" in args.parts and size != 1000:
                    ms = {"fill": [], "encrypt_zeros": []}
                    for rnd in range(args.rounds + 1):
                        ctx.pool_reserve(size)             # an empty ring
                        torch.cuda.synchronize()
                        t = timed(lambda: chk(lib.pai_pool_fill_dev(ctx.handle, size, N.PAI_OBF_RNG, None, 0, 0, RK, 0,
                                                                    stream.cuda_stream)))
                        u = timed(lambda: rng_call(ctx, b, b.zeros, N.PAI_I64))
                        if rnd:
                            ms["fill"].append(t)
                            ms["encrypt_zeros"].append(u)
                    row = {"party": name, "size": size, "fill": stats(ms["fill"], size),
                           "encrypt_zeros": stats(ms["encrypt_zeros"], size)}
                    row["split_ms"] = round(row["fill"]["median_ms"] - row["encrypt_zeros"]["median_ms"], 4)
                    row["split_share_of_fill"] = round(row["split_ms"] / row["fill"]["median_ms"], 4)
                    rows_c.append(row)
                    print(json.dumps(row), flush=True)
                ctx.pool_reserve(0)
                del b
                torch.cuda.empty_cache()
        if "b" in args.parts:
            result["b_pooled_vs_rng"] = rows_b
        if "c" in args.parts:
            result["c_fill_cost"] = rows_c

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
