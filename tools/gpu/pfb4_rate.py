#!/usr/bin/env python3
"""Break-even inputs of the 2049..4096-bit public fixed-base sampler (kernels_pfb4.hpp) on one device: a public-key-only
party's 262 144 float32 elements under device RNG (device-resident buffers, warm, median of 5 calls after one discarded;
k_pe4_*: of 3 after one, a call takes seconds) on k_pe4_* (PAI_OPT_PUBLIC_FB = 1, the default) and on k_pfb4 (= 2) at the
windows 12 and 16, on the 4096-bit key of tests/golden/pfb4_keys.json, with the stage times and the wall time of
pai_ctx_public_fb_prepare (first build of the context, then a rebuild on pooled memory). One JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import torch  # noqa: E402


def main():
    from flex.crypto.paillier import _native as N
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << 18
    with open(os.path.join(ROOT, "tests", "golden", "pfb4_keys.json")) as f:
        pub = int(json.load(f)["keys"]["4096_top_limb_full"]["n"], 16)
    x = torch.randn(n, dtype=torch.float32, device=dev)
    ct = torch.empty((n, 256), dtype=torch.int32, device=dev)
    ex = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.load_library()
    row = {"nb": 4096, "n": n, "device": torch.cuda.get_device_name(dev)}

    def rate(c, calls):
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.pai_encrypt_dev(c.handle, N.PAI_F32, x.data_ptr(), n, 0, 0, N.PAI_OBF_RNG, None, 0, 0, bytes(32), 0,
                                     ct.data_ptr(), ex.data_ptr(), st.data_ptr(), stream.cuda_stream)
            assert rc == 0, lib.pai_last_error()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        ms = statistics.median(times[1:])
        return {"ms": round(ms * 1e3, 2), "min_ms": round(min(times[1:]) * 1e3, 2), "max_ms": round(max(times[1:]) * 1e3, 2),
                "encrypts_per_s": round(n / ms), "stages_ms": [round(v, 2) for v in c.stage_times()]}

    c = N.Context(pub, 0)
    c.set_stage_timing(True)
    row["k_pe4"] = rate(c, 4)
    c.close()
    for w in (12, 16):
        c = N.Context(pub, 0)
        c.set_public_fixed_base(2)
        c.set_pfb_window(w)
        c.set_stage_timing(True)
        builds = []
        for _ in range(2):
            c.set_pfb_window(16 if w == 12 else 12)   # drops the tables
            c.set_pfb_window(w)
            t0 = time.perf_counter()
            c.prepare_public_fixed_base()
            builds.append(round(time.perf_counter() - t0, 4))
        r = rate(c, 6)
        r["build_s"] = builds
        _, K, W, _ = c.public_fixed_base_info()
        r["rows"] = K << W
        row[f"k_pfb4_w{w}"] = r
        c.close()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
