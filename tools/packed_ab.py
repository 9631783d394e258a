#!/usr/bin/env python3
"""A/B of packed plaintexts against one value per ciphertext, in one process on one GPU, on a 2048-bit key holder with
its default-window fixed-base tables resident, over 2^20 float32 values (device buffers, HIP events on the current stream):
a = pai_encrypt_packed_dev -> 2-way pai_add_dev -> pai_decrypt_packed_dev on ceil(N / slots) ciphertexts;
b = the same values through pai_encrypt_dev (fixed exponent) -> 2-way pai_add_dev -> pai_decrypt_dev on N ciphertexts.
Layouts: (slot_bits, value_bits, exponent) = (32, 24, 5) with 63 slots and (64, 53, 10) with 31. One warm-up pass per
side, then --rounds rounds that alternate a and b, every stage timed on its own. Both sides must decode to the same
numbers (x + x at the layout's exponent): checked once per layout. Writes values/s per stage and side to
profiles/packed_ab.json (--out) and prints them.

    python tools/packed_ab.py [--rounds 3] [--size 1048576] [--nb 2048] [--out profiles/packed_ab.json]
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

RK = bytes(range(32))
LAYOUTS = ((32, 24, 5), (64, 53, 10))
STAGES = ("encrypt", "add", "decrypt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--nb", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        k = json.load(f)["keys"][str(args.nb)]
    n, p, q = int(k["n"], 16), int(k["p"], 16), int(k["q"], 16)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    lib = N.load_library()
    ctx = N.Context(n, 0, p, q)
    ctx.prepare_fixed_base()
    W, size = ctx.ct_words, args.size
    x = (torch.rand(size, generator=torch.Generator().manual_seed(1)) * 8 - 4).to(torch.float32).to(dev)

    def chk(rc):
        assert rc == 0, lib.pai_last_error()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    result = {"device": torch.cuda.get_device_name(dev), "nb": args.nb, "values": size, "rounds": args.rounds,
              "fb_window": ctx.fb_window, "layouts": []}
    for sb, vb, e in LAYOUTS:
        slots = ctx.pack_max_slots(sb)
        lay = N.pack_layout((sb, vb, e, slots))
        C = -(-size // slots)
        # side a: C ciphertexts; side b: `size` ciphertexts. The add's operands are [2][n][W]: the encryption goes into
        # operand 0 and is copied to operand 1 outside the timed stages (x + x)
        ops = {"a": torch.empty((2, C, W), dtype=torch.int32, device=dev),
               "b": torch.empty((2, size, W), dtype=torch.int32, device=dev)}
        cnt = {"a": C, "b": size}
        exps = {sd: torch.full((2, cnt[sd]), e, dtype=torch.int32, device=dev) for sd in "ab"}
        out = {sd: torch.empty((cnt[sd], W), dtype=torch.int32, device=dev) for sd in "ab"}
        oe = {sd: torch.empty(cnt[sd], dtype=torch.int32, device=dev) for sd in "ab"}
        st = torch.empty(size, dtype=torch.int32, device=dev)
        val = {sd: torch.empty(size, dtype=torch.float64, device=dev) for sd in "ab"}
        mant = torch.empty(size, dtype=torch.int64, device=dev)
        dst = torch.empty(size, dtype=torch.int32, device=dev)

        def stage(sd, name):
            if name == "encrypt" and sd == "a":
                chk(lib.pai_encrypt_packed_dev(ctx.handle, N.PAI_F32, x.data_ptr(), size, ctypes.byref(lay), N.PAI_OBF_RNG,
                                               None, 0, 0, RK, 0, ops["a"][0].data_ptr(), st.data_ptr(), s))
            elif name == "encrypt":
                chk(lib.pai_encrypt_dev(ctx.handle, N.PAI_F32, x.data_ptr(), size, N.PAI_EXP_FIXED, e, N.PAI_OBF_RNG, None,
                                        0, 0, RK, 0, ops["b"][0].data_ptr(), exps["b"][0].data_ptr(), st.data_ptr(), s))
            elif name == "add":
                chk(lib.pai_add_dev(ctx.handle, ops[sd].data_ptr(), exps[sd].data_ptr(), 2, cnt[sd], out[sd].data_ptr(),
                                    oe[sd].data_ptr(), s))
            elif sd == "a":
                chk(lib.pai_decrypt_packed_dev(ctx.handle, out["a"].data_ptr(), ctypes.byref(lay), size,
                                               val["a"].data_ptr(), mant.data_ptr(), dst.data_ptr(), s))
            else:
                chk(lib.pai_decrypt_dev(ctx.handle, out["b"].data_ptr(), oe["b"].data_ptr(), size, val["b"].data_ptr(),
                                        mant.data_ptr(), dst.data_ptr(), None, s))

        def run(sd, ms=None):
            for name in STAGES:
                t = timed(lambda: stage(sd, name))
                if ms is not None:
                    ms[sd][name].append(t)
                if name == "encrypt":
                    assert int(st.count_nonzero()) == 0
                    ops[sd][1].copy_(ops[sd][0])

        run("a")                                           # warm-up, and the outputs of the comparison
        run("b")
        torch.cuda.synchronize()
        want = (x.double() * 16.0 ** e).round() * 2 * 16.0 ** -e       # rint(x 16^e) is exact in float64 here
        same = bool(torch.equal(val["a"], val["b"])) and bool(torch.equal(val["a"], want))
        ms = {sd: {name: [] for name in STAGES} for sd in "ab"}
        for _ in range(args.rounds):
            run("a", ms)
            run("b", ms)
        row = {"slot_bits": sb, "value_bits": vb, "exponent": e, "slots": slots, "ciphertexts": {"a": C, "b": size},
               "outputs_equal": same}
        for sd in "ab":
            row[sd] = {}
            for name in STAGES:
                med = statistics.median(ms[sd][name])
                row[sd][name] = {"ms": [round(v, 3) for v in ms[sd][name]], "median_ms": round(med, 3),
                                 "values_per_s": round(size / med * 1e3)}
            tot = sum(row[sd][name]["median_ms"] for name in STAGES)
            row[sd]["total"] = {"median_ms": round(tot, 3), "values_per_s": round(size / tot * 1e3)}
        row["a_over_b"] = {name: round(row["a"][name]["values_per_s"] / row["b"][name]["values_per_s"], 2)
                           for name in STAGES + ("total",)}
        result["layouts"].append(row)
        print(f"({sb}, {vb}, {e}) x {slots}: outputs equal {same}; values/s a vs b: " +
              ", ".join(f"{name} {row['a'][name]['values_per_s']:.3g} vs {row['b'][name]['values_per_s']:.3g}"
                        for name in STAGES + ("total",)), flush=True)
        del ops, exps, out, oe, st, val, mant, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
