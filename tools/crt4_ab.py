#!/usr/bin/env python3
"""A/B of a 4096-bit key holder's explicit-r encryption above the rows, in one process, one library and ONE context on
one GPU: a = the split-pair CRT (kernels_crt4.hpp: k_crt4_pre + k_crt4_a, k_crt4_b, k_crt_fin<8>), b = the same calls
with PAI_OPT_CRT_ENCRYPT = 0, i.e. k_encrypt<8> (the kernel they ran on before, unchanged). The context has the fixed
bases off, rows_max 0 and crt4_min 0; the inputs are device-resident float32 with a distinct obfuscator per element
(PAI_OBF_GIVEN, ct_words random words each). Per size (262 144, and 128 and 256 around the default floor): one warm-up
call per path, then three rounds that alternate a and b; every timing ends in a device synchronise. Writes the rates,
their spread, each path's stage times, the model's lane-MAC counts (tools/crt4_model.py) with each new kernel's share of
the integer-MAC peak, and the library's sha256 to profiles/crt4_ab.json (--out), and prints the same JSON line.

    python tools/crt4_ab.py [--sizes 262144,128,256] [--rounds 3] [--out profiles/crt4_ab.json] [--lib other.so]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

INT_MAC_PEAK = 35.13e12      # lane-MACs/s: the integer multiply-add peak DESIGN.md uses


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="262144,128,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crt4_ab.json"))
    ap.add_argument("--lib", default=None, help="another build of libflexpai.so (a measurement build, e.g. "
                    "-DFPAI_CRT4_OCC_B=2); default: the product library")
    args = ap.parse_args()
    import crt4_model
    from flex.crypto.paillier import _native as N
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        k = json.load(f)["keys"]["4096"]
    key_n, key_p, key_q = (int(k[v], 16) for v in ("n", "p", "q"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    lib_path = os.path.abspath(args.lib) if args.lib else N.LIB_PATH
    lib = N.load_library(lib_path) if args.lib else N.load_library()
    c = N.Context(key_n, 0, key_p, key_q, lib=lib if args.lib else None)
    c.set_fixed_base(False)
    c.set_rows_max(0)
    c.set_crt4_min(0)
    c.set_stage_timing(True)
    assert c.pair_paths & 8
    W = c.ct_words
    mac_a, mac_b, mac_e8 = crt4_model.mac_count(*sorted((key_p, key_q)))
    row = {"nb": 4096, "rounds": args.rounds, "sizes": {},
           "model": {"lane_macs_stage_a": mac_a, "lane_macs_stage_b": mac_b, "lane_macs_k_encrypt8": mac_e8,
                     "ratio": round(mac_e8 / (mac_a + mac_b), 3)}}
    for n in (int(v) for v in args.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        x = torch.randn(n, dtype=torch.float32, device=dev, generator=g)
        r = torch.randint(-2 ** 31, 2 ** 31, (n, W), dtype=torch.int32, device=dev, generator=g)
        ex = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        ct = {name: torch.empty((n, W), dtype=torch.int32, device=dev) for name in ("a", "b")}

        def call(name):
            c.set_crt(name == "a")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.pai_encrypt_dev(c.handle, N.PAI_F32, x.data_ptr(), n, 0, 0, N.PAI_OBF_GIVEN, r.data_ptr(), W, W, None, 0,
                                     ct[name].data_ptr(), ex.data_ptr(), st.data_ptr(), stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, c.stage_times()

        for name in ("a", "b"):
            call(name)                               # warm-up: scratch and work buffers, code objects
        times = {"a": [], "b": []}
        stages = {"a": [], "b": []}
        for _ in range(args.rounds):
            for name in ("a", "b"):
                t, s = call(name)
                times[name].append(t)
                stages[name].append(s)
        res = {"identical": bool(torch.equal(ct["a"], ct["b"]))}
        for name in ("a", "b"):
            ms = [t * 1e3 for t in times[name]]
            med = statistics.median(ms)
            res[name] = {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
                         "encrypts_per_s": round(n / med * 1e3), "spread": round((max(ms) - min(ms)) / med, 4),
                         "stages_ms": [[round(v, 3) for v in s] for s in stages[name]]}
        res["ratio_a_over_b"] = round(res["a"]["encrypts_per_s"] / res["b"]["encrypts_per_s"], 3)
        sa, sb = (statistics.median(s[i] for s in stages["a"]) for i in (0, 1))
        res["stage_a_share_of_int_mac_peak"] = round(mac_a * n / sa * 1e3 / INT_MAC_PEAK, 4)
        res["stage_b_share_of_int_mac_peak"] = round(mac_b * n / sb * 1e3 / INT_MAC_PEAK, 4)
        row["sizes"][str(n)] = res
        del x, r, ex, st, ct
    c.set_crt(True)
    row["sha256"] = {os.path.basename(lib_path): sha256(lib_path)}
    row["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
