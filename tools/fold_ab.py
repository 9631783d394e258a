#!/usr/bin/env python3
"""A/B of pai_pack_ciphertexts against the only route the library had before it, in one process on one GPU, device
buffers, HIP events on the current stream. Per configuration (key bits, slot bits, slots) = (2048, 32, 63) and
(1024, 32, 31), over 2^18 ordinary ciphertexts of small integers (device RNG, exponent 0):

a = pai_pack_ciphertexts_dev of the N ciphertexts into C = ceil(N / slots) packed ones;
b = the chain that gives the same bits: slots - 1 rounds of pai_mul_dev by 2^slot_bits and a 2-way pai_add_dev over
    C ciphertexts. The chain needs its operands slot-major ([slots][C][W], the missing slots of the last output filled
    with the ciphertext 1); that transpose is made once, outside the timed region, and only the copy of a round's slot
    into the add's second operand (C rows) is timed with the chain;
c = pai_decrypt_dev of the N ordinary ciphertexts, against a + pai_decrypt_packed_dev of the C packed ones.

One warm-up pass, then --rounds rounds that alternate a, b and the two decrypts; medians. a and b must give identical
words and both decrypts the input integers: checked once per configuration. Also reported: the fold's multiply-accumulate
rate (C outputs x ((slots - 1) slot_bits + 2 slots + 1) Montgomery products x 2 S^2 lane-MACs, S = 37 x lanes per group)
against the chip's 35.13 T lane-MAC/s scaled to the SIMDs the call's blocks occupy, and the bytes per value of the
ciphertext words on the wire. Writes profiles/fold_ab.json (--out) and prints it.

    python tools/fold_ab.py [--rounds 3] [--size 262144] [--out profiles/fold_ab.json]

--rows: the A/B of the fold's two kernels instead, k_pack_fold_w on 16-lane rows against k_pack_fold on lane groups, for
the threshold of PAI_OPT_FOLD_ROWS (include/flexpai.h PAI_FOLD_ROWS_MAX_*). One process, one library, public contexts;
the two paths alternate through PAI_OPT_FOLD_ROWS = 0 / 2 and PAI_OPT_FOLD_PATH is checked after every call; HIP events
around pai_pack_ciphertexts_dev (32-bit slots, k = 63, or the 31 that fit a 1024-bit key) and pai_repack_dev (s = 2,
sb = 48, the largest g) on a side stream; one warm-up pass, then --rounds rounds, medians; 64, 1 024, 4 096, 16 384 and
65 536 outputs (--counts) at 1024, 2048 and 4096 bits (--bits). The inputs are random residues below n^2 (the chains do
not depend on the data); the two paths' outputs are compared once per cell. Per key size and entry point the table
gives rows / groups and the largest count at which the rows are more than 5 % faster; the result is merged into --out
under "rows_ab" (the record above stays).

    python tools/fold_ab.py --rows [--rounds 3] [--bits 1024,2048,4096] [--counts 64,1024,4096,16384,65536]
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
CONFIGS = ((2048, 32, 63), (1024, 32, 31))
PEAK_LANE_MACS = 35.13e12          # the chip's integer multiply-accumulate peak, 1024 SIMDs
TPI = {1024: 2, 2048: 4, 4096: 8}


def rows_ab(args):
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    lib = N.load_library()
    counts = [int(v) for v in args.counts.split(",")]
    result = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "counts": counts, "margin": 0.05,
              "keys": {}}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0)
        W = ctx.ct_words
        k = min(63, (nb - 2) // 32)
        g = (nb - 2) // 48 // 2
        entries = {"pack_ciphertexts": (k, N.pack_layout((32, 32, 0, k))), "repack": (g, N.pack_layout((48, 48, 0, 2)))}
        most = max(counts) * max(k, g)
        gen = torch.Generator(device=dev).manual_seed(nb)
        ct = torch.randint(-(1 << 31), (1 << 31) - 1, (most, W), generator=gen, dtype=torch.int32, device=dev)
        ct[:, W - 1] = 0                                       # below 2^(32 (W - 1)) < n^2
        ex = torch.zeros(most, dtype=torch.int32, device=dev)
        outs = {m: torch.empty((max(counts), W), dtype=torch.int32, device=dev) for m in (0, 2)}
        torch.cuda.synchronize()
        per_key = {}
        for name, (per, lay) in entries.items():
            cells = []
            for C in counts:
                n_in = C * per

                def call(mode):
                    ctx.set_fold_rows(mode)
                    if name == "repack":
                        rc = lib.pai_repack_dev(ctx.handle, ct.data_ptr(), n_in, ctypes.byref(lay), per,
                                                outs[mode].data_ptr(), s)
                    else:
                        rc = lib.pai_pack_ciphertexts_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n_in, ctypes.byref(lay),
                                                          outs[mode].data_ptr(), None, s)
                    assert rc == 0, lib.pai_last_error()
                    assert ctx.fold_path == (2 if mode == 2 else 1)

                ms = {0: [], 2: []}
                for rnd in range(args.rounds + 1):             # round 0 is the warm-up
                    for mode in (0, 2):
                        t = timed(lambda: call(mode))
                        if rnd:
                            ms[mode].append(t)
                same = bool(torch.equal(outs[0][:C], outs[2][:C]))
                grp, row = statistics.median(ms[0]), statistics.median(ms[2])
                cell = {"outputs": C, "inputs_per_output": per, "same_words": same,
                        "groups_ms": [round(v, 3) for v in ms[0]], "rows_ms": [round(v, 3) for v in ms[2]],
                        "groups_median_ms": round(grp, 3), "rows_median_ms": round(row, 3),
                        "rows_over_groups": round(row / grp, 3)}
                cells.append(cell)
                print(json.dumps({"nb": nb, "entry": name, **cell}), flush=True)
            wins = [c["outputs"] for c in cells if c["rows_median_ms"] < (1 - result["margin"]) * c["groups_median_ms"]]
            per_key[name] = {"cells": cells, "rows_max": max(wins) if wins else 0}
        per_key["rows_max"] = min(v["rows_max"] for v in per_key.values())
        result["keys"][str(nb)] = per_key
        ctx.set_fold_rows(1)
        ctx.close()
        del ct, ex, outs
        torch.cuda.empty_cache()
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged["rows_ab"] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps({nb: v["rows_max"] for nb, v in result["keys"].items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=1 << 18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_ab.json"))
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--bits", default="1024,2048,4096")
    ap.add_argument("--counts", default="64,1024,4096,16384,65536")
    args = ap.parse_args()
    if args.rows:
        return rows_ab(args)
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    lib = N.load_library()
    size = args.size

    def chk(rc):
        assert rc == 0, lib.pai_last_error()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    result = {"device": torch.cuda.get_device_name(dev), "values": size, "rounds": args.rounds, "configs": []}
    for nb, sb, slots in CONFIGS:
        k = keys[str(nb)]
        ctx = N.Context(int(k["n"], 16), 0, int(k["p"], 16), int(k["q"], 16))
        W = ctx.ct_words
        assert slots == ctx.pack_max_slots(sb)
        lay = N.pack_layout((sb, sb, 0, slots))
        C = -(-size // slots)
        x = torch.randint(-(1 << 20), 1 << 20, (size,), generator=torch.Generator().manual_seed(nb), dtype=torch.int64)
        d_x = x.to(dev)
        ct = torch.empty((size, W), dtype=torch.int32, device=dev)
        ex = torch.empty(size, dtype=torch.int32, device=dev)
        st = torch.empty(size, dtype=torch.int32, device=dev)
        chk(lib.pai_encrypt_dev(ctx.handle, N.PAI_I64, d_x.data_ptr(), size, N.PAI_EXP_AUTO, 0, N.PAI_OBF_RNG, None, 0, 0,
                                RK, 0, ct.data_ptr(), ex.data_ptr(), st.data_ptr(), s))
        torch.cuda.synchronize()
        assert int(st.count_nonzero()) == 0 and int(ex.count_nonzero()) == 0
        # slot-major operands of the chain, the tail of the last output filled with the ciphertext 1
        padded = torch.zeros((C * slots, W), dtype=torch.int32, device=dev)
        padded[:, 0] = 1
        padded[:size] = ct
        by_slot = padded.view(C, slots, W).transpose(0, 1).contiguous()
        del padded
        ex_c = torch.zeros(C, dtype=torch.int32, device=dev)
        ex_2 = torch.zeros((2, C), dtype=torch.int32, device=dev)
        pair = torch.empty((2, C, W), dtype=torch.int32, device=dev)
        acc = torch.empty((C, W), dtype=torch.int32, device=dev)
        e_tmp = torch.empty(C, dtype=torch.int32, device=dev)
        st_c = torch.empty(C, dtype=torch.int32, device=dev)
        scalar = torch.tensor([1 << sb], dtype=torch.int64, device=dev)
        folded = torch.empty((C, W), dtype=torch.int32, device=dev)
        val = torch.empty(size, dtype=torch.float64, device=dev)
        mant = {sd: torch.empty(size, dtype=torch.int64, device=dev) for sd in ("plain", "packed")}
        dst = torch.empty(size, dtype=torch.int32, device=dev)

        def fold():
            chk(lib.pai_pack_ciphertexts_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), size, ctypes.byref(lay),
                                             folded.data_ptr(), st.data_ptr(), s))

        def chain():
            src = by_slot[slots - 1]
            for j in range(slots - 2, -1, -1):
                chk(lib.pai_mul_dev(ctx.handle, src.data_ptr(), ex_c.data_ptr(), C, N.PAI_I64, scalar.data_ptr(), 0,
                                    pair[0].data_ptr(), e_tmp.data_ptr(), st_c.data_ptr(), s))
                pair[1].copy_(by_slot[j])
                chk(lib.pai_add_dev(ctx.handle, pair.data_ptr(), ex_2.data_ptr(), 2, C, acc.data_ptr(), e_tmp.data_ptr(), s))
                src = acc

        def decrypt_plain():
            chk(lib.pai_decrypt_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), size, val.data_ptr(),
                                    mant["plain"].data_ptr(), dst.data_ptr(), None, s))

        def decrypt_packed():
            chk(lib.pai_decrypt_packed_dev(ctx.handle, folded.data_ptr(), ctypes.byref(lay), size, val.data_ptr(),
                                           mant["packed"].data_ptr(), dst.data_ptr(), s))

        sides = (("fold", fold), ("chain", chain), ("decrypt_plain", decrypt_plain), ("decrypt_packed", decrypt_packed))
        for _, fn in sides:                                    # warm-up, and the outputs of the comparison
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(folded, acc)) and int(st.count_nonzero()) == 0
        decoded = bool(torch.equal(mant["plain"], d_x)) and bool(torch.equal(mant["packed"], d_x))
        ms = {name: [] for name, _ in sides}
        for _ in range(args.rounds):
            for name, fn in sides:
                ms[name].append(timed(fn))
        med = {name: statistics.median(v) for name, v in ms.items()}
        S = 37 * TPI[nb]
        products = (slots - 1) * sb + 2 * slots + 1
        blocks = min(-(-C // (256 // TPI[nb])), 2 * torch.cuda.get_device_properties(dev).multi_processor_count)
        simds = min(4 * blocks, 1024)
        macs = C * products * 2 * S * S
        row = {"nb": nb, "slot_bits": sb, "slots": slots, "ciphertexts": {"in": size, "out": C},
               "fold_equals_chain": same, "decrypts_equal_inputs": decoded,
               "ms": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
               "median_ms": {name: round(v, 3) for name, v in med.items()},
               "fold_over_chain": round(med["fold"] / med["chain"], 3),
               "fold_values_per_s": round(size / med["fold"] * 1e3),
               "decrypt_plain_values_per_s": round(size / med["decrypt_plain"] * 1e3),
               "fold_plus_decrypt_packed_ms": round(med["fold"] + med["decrypt_packed"], 3),
               "fold_plus_decrypt_packed_values_per_s": round(size / (med["fold"] + med["decrypt_packed"]) * 1e3),
               "decrypt_speedup": round(med["decrypt_plain"] / (med["fold"] + med["decrypt_packed"]), 2),
               "fold_products_per_output": products, "fold_blocks": blocks,
               "fold_lane_macs_per_s": round(macs / med["fold"] * 1e3),
               "fold_share_of_mac_peak_on_its_simds": round(macs / med["fold"] * 1e3 / (PEAK_LANE_MACS * simds / 1024), 3),
               "wire_bytes_per_value": {"ordinary": 4 * W + 5, "packed": round(4 * W * C / size, 2)}}
        result["configs"].append(row)
        print(json.dumps(row), flush=True)
        del ct, by_slot, pair, acc, folded, val, mant, dst
        torch.cuda.empty_cache()
    if os.path.exists(args.out):                               # the record of --rows stays
        with open(args.out) as f:
            result.update({k: v for k, v in json.load(f).items() if k == "rows_ab"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
