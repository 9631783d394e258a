#!/usr/bin/env python3
"""A/B of the array re-randomisation (pai_obfuscate_dev), in one process on one GPU, on a 2048-bit key holder with its
fixed-base tables built:
a = pai_obfuscate_dev in place (kernels_obf.hpp: r^n by the encrypt route, then k_obf_mul);
b = what the public calls could already do: pai_encrypt_dev of int64 zeros into a buffer, then a two-operand
    pai_add_dev of the ciphertexts and that buffer with one shared (all-zero) exponent array.
Sizes: 2^20 device-resident elements and 1 000 (--sizes). Ciphertexts are random words below n^2. One warm-up call per
side, then --rounds rounds that alternate a and b; every call is timed by HIP events on the current stream. Both sides
use the same rng key and index base, so their outputs must be identical (the bits contract of include/flexpai.h):
checked once per size. Once, the per-element path is timed too: obfuscator.apply_obfuscation over 256 ciphertexts.
Writes the times, their spread, elements/s and the verdict to profiles/obf_ab.txt (--out) and prints them.

    python tools/obf_ab.py [--rounds 3] [--sizes 1048576,1000] [--nb 2048] [--out profiles/obf_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402

RK = bytes(range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="1048576,1000")
    ap.add_argument("--nb", type=int, default=2048)
    ap.add_argument("--loop", type=int, default=256, help="elements of the per-element apply_obfuscation loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obf_ab.txt"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        k = json.load(f)["keys"][str(args.nb)]
    n, p, q = int(k["n"], 16), int(k["p"], 16), int(k["q"], 16)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library()
    ctx = N.Context(n, 0, p, q)
    ctx.prepare_fixed_base()
    W = ctx.ct_words
    lines = [f"obf_ab: {torch.cuda.get_device_name(dev)}, nb = {args.nb}, key holder, fixed-base window {ctx.fb_window}, "
             f"{args.rounds} interleaved rounds",
             "a = pai_obfuscate_dev in place; b = pai_encrypt_dev(int64 zeros) + 2-operand pai_add_dev"]
    rows = []
    for size in [int(v) for v in args.sizes.split(",") if v]:
        g = torch.Generator(device=dev).manual_seed(size)
        ops = torch.randint(0, 2 ** 31 - 1, (2, size, W), dtype=torch.int32, device=dev, generator=g)
        ops[:, :, W - 1] = 0                               # < 2^(32 (W - 1)) < n^2
        ct, e0 = ops[0], ops[1]
        orig = ct.clone()
        work = ct.clone()                                  # side a re-randomises this one in place, call after call
        zeros = torch.zeros(size, dtype=torch.int64, device=dev)
        exps = torch.zeros((2, size), dtype=torch.int32, device=dev)
        st = torch.empty(size, dtype=torch.int32, device=dev)
        out_b = torch.empty((size, W), dtype=torch.int32, device=dev)
        oe_b = torch.empty(size, dtype=torch.int32, device=dev)

        def run_a(buf):
            rc = lib.pai_obfuscate_dev(ctx.handle, buf.data_ptr(), size, N.PAI_OBF_RNG, None, 0, 0, RK, 0, buf.data_ptr(),
                                       stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()

        def run_b():
            rc = lib.pai_encrypt_dev(ctx.handle, N.PAI_I64, zeros.data_ptr(), size, N.PAI_EXP_AUTO, 0, N.PAI_OBF_RNG, None,
                                     0, 0, RK, 0, e0.data_ptr(), exps[1].data_ptr(), st.data_ptr(), stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()
            rc = lib.pai_add_dev(ctx.handle, ops.data_ptr(), exps.data_ptr(), 2, size, out_b.data_ptr(), oe_b.data_ptr(),
                                 stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1)

        check = orig.clone()
        run_a(check)                                       # warm-up of a, and the identity check against b
        run_b()                                            # warm-up of b
        torch.cuda.synchronize()
        identical = bool(torch.equal(check, out_b))
        ms = {"a": [], "b": []}
        for _ in range(args.rounds):
            ms["a"].append(timed(lambda: run_a(work)))
            ms["b"].append(timed(run_b))
        row = {"size": size, "identical": identical}
        for s in "ab":
            med = statistics.median(ms[s])
            row[s] = {"ms": [round(v, 3) for v in ms[s]], "median_ms": round(med, 3),
                      "spread": round((max(ms[s]) - min(ms[s])) / med, 4), "elems_per_s": round(size / med * 1e3)}
        row["b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
        # no slower, the spread of the interleaved repeats being the margin
        row["a_no_slower"] = bool(min(ms["a"]) <= max(ms["b"]))
        row["a_faster_beyond_spread"] = bool(max(ms["a"]) < min(ms["b"]))
        rows.append(row)
        for s in "ab":
            lines.append(f"N = {size:>8}  {s}: {row[s]['ms']} ms, median {row[s]['median_ms']} ms, spread "
                         f"{row[s]['spread']}, {row[s]['elems_per_s']} elements/s")
        lines.append(f"N = {size:>8}  b / a = {row['b_over_a']}, a no slower than b within the spread: {row['a_no_slower']}, "
                     f"a faster beyond the spread: {row['a_faster_beyond_spread']}, outputs identical: {identical}")
        del ops, ct, e0, orig, work, zeros, exps, st, out_b, oe_b, check
        torch.cuda.empty_cache()
    # the per-element path: one host-buffer encryption of an int64 zero per ciphertext (obfuscator.obfuscator_power)
    from flex.crypto.paillier.api import generate_paillier_decryptor
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.obfuscator import apply_obfuscation
    pk = PaillierPublicKey(n)
    generate_paillier_decryptor(n, p, q)
    cs = [pow(n + 1, i + 2, n * n) for i in range(args.loop)]
    apply_obfuscation(cs[0], pk)                           # the package context of this key, its tables
    t0 = time.perf_counter()
    for c in cs:
        apply_obfuscation(c, pk)
    loop_s = time.perf_counter() - t0
    lines.append(f"per-element apply_obfuscation over {args.loop} ciphertexts: {loop_s * 1e3:.1f} ms, "
                 f"{loop_s / args.loop * 1e6:.0f} us per element, {args.loop / loop_s:.0f} elements/s")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    print(json.dumps({"rows": rows, "loop_us_per_element": round(loop_s / args.loop * 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
