#!/usr/bin/env python3
"""A/B of PAI_OPT_PRIME_LIMBS on a 3072-bit key holder, in one process on one GPU:
a = the option at 1 (k_dec4_*<56>, k_crt4_*<56>, and k_dec_w / k_crt_w<56, 112> on the rows),
b = the option at 0 (the same kernels at 74 / 148 limbs: the path every such key took before the option),
for pai_decrypt_dev and pai_encrypt_dev with explicit r, above the rows on --n elements (PAI_OPT_ROWS_MAX = 0,
PAI_OPT_CRT4_MIN = 0) and on the rows on --rows-n elements. Device-resident buffers, HIP events around each call, one
warm-up call per side, then --rounds rounds that alternate a and b. --alt LIB adds side c: the option at 1 on another
build of the library (a measurement build with other occupancies). Checks that all sides give the same words, writes the
times, their spread, the ratios b / a and the stage times to --out and prints the same JSON line.

    python tools/prime_limbs_ab.py [--n 262144] [--rows-n 1000] [--rounds 3] [--alt LIB] [--out profiles/prime_limbs_ab.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--rows-n", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alt", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prime_limbs_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    from oracle import paillier_oracle as O
    key_n, p, q = O.generate_keypair(3072, seed=5)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    nmax = max(args.n, args.rows_n)
    gen = torch.Generator(device=dev).manual_seed(3072)
    x = torch.randn(nmax, dtype=torch.float32, device=dev, generator=gen)
    side = {}
    for name, opt, path in (("a", True, None), ("b", False, None), ("c", True, args.alt)):
        if name == "c" and not path:
            continue
        lib = N.load_library(path) if path else N.load_library()
        c = N.Context(key_n, 0, lib=lib)
        c.set_prime_limbs(opt)
        c.set_private(p, q)
        c.set_stage_timing(True)
        assert c.prime_limbs == (56 if opt else 0) and c.pair_paths == 9
        side[name] = {"lib": lib, "ctx": c, "ct": torch.empty((nmax, c.ct_words), dtype=torch.int32, device=dev),
                      "val": torch.empty(nmax, dtype=torch.float64, device=dev)}
    c0 = side["a"]["ctx"]
    rw = c0.pt_words                                  # explicit r: pt_words random words per element (any r < 2^(32 rw))
    r = torch.randint(-2 ** 31, 2 ** 31 - 1, (nmax, rw), dtype=torch.int32, device=dev, generator=gen)
    ex = torch.empty(nmax, dtype=torch.int32, device=dev)
    st = torch.empty(nmax, dtype=torch.int32, device=dev)
    mant = torch.empty(nmax, dtype=torch.int64, device=dev)

    def call(name, what, n):
        s = side[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if what == "encrypt":
            rc = s["lib"].pai_encrypt_dev(s["ctx"].handle, N.PAI_F32, x.data_ptr(), n, 0, 0, N.PAI_OBF_GIVEN, r.data_ptr(),
                                          rw, rw, None, 0, s["ct"].data_ptr(), ex.data_ptr(), st.data_ptr(),
                                          stream.cuda_stream)
        else:
            rc = s["lib"].pai_decrypt_dev(s["ctx"].handle, s["ct"].data_ptr(), ex.data_ptr(), n, s["val"].data_ptr(),
                                          mant.data_ptr(), st.data_ptr(), None, stream.cuda_stream)
        assert rc == 0, s["lib"].pai_last_error()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), s["ctx"].stage_times()

    row = {"nb": 3072, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "sides": sorted(side)}
    for label, n, rows_max, crt4_min in (("above", args.n, 0, 0), ("rows", args.rows_n, 4096, 128)):
        for s in side.values():
            s["ctx"].set_rows_max(rows_max)
            s["ctx"].set_crt4_min(crt4_min)
        res = {"n": n}
        for what in ("encrypt", "decrypt"):           # decrypt reads the ciphertexts its side's encrypt left
            for name in side:
                call(name, what, n)                   # warm-up: scratch and work buffers, code objects
            ms, stages = {k: [] for k in side}, {k: [] for k in side}
            for _ in range(args.rounds):
                for name in side:
                    t, sg = call(name, what, n)
                    ms[name].append(t)
                    stages[name].append(sg)
            out = side["a"]["ct"] if what == "encrypt" else side["a"]["val"]
            same = all(torch.equal(out[:n], (s["ct"] if what == "encrypt" else s["val"])[:n]) for s in side.values())
            res[what] = {"identical": bool(same)}
            for name in side:
                med = statistics.median(ms[name])
                res[what][name] = {"ms": [round(v, 3) for v in ms[name]], "median_ms": round(med, 3),
                                   "per_s": round(n / med * 1e3), "spread": round((max(ms[name]) - min(ms[name])) / med, 4),
                                   "stages_ms": [[round(v, 3) for v in sg] for sg in stages[name]]}
            res[what]["ratio_b_over_a"] = round(res[what]["b"]["median_ms"] / res[what]["a"]["median_ms"], 3)
            res[what]["every_a_faster_than_every_b"] = max(ms["a"]) < min(ms["b"])
        row[label] = res
    line = json.dumps(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
