#!/usr/bin/env python3
"""A/B of the index lists on the device, in one process on one GPU, public-key contexts:
(a) segment sums: a = pai_segment_add_idx_dev of this library over lists that are resident (uploaded before the clock
    starts); b = pai_segment_add_dev of a library built from the parent commit (--parent; this library's when the file
    is absent: the host-list call is unchanged) over the same lists as host arrays. 262 144 ciphertexts, 512 segments of
    512 members (a random permutation cut into ranges), and one shape of SHORT segments, 65 536 segments of 4 members,
    where the resident path plans more levels than the host path needs;
(b) take: pai_take_idx_dev against pai_take_dev for M = 262 144 (a permutation);
(c) one boosting level through the Python layer: DeviceCiphertextBuffer.histogram -> cumsum over 262 144 x 16 features x
    32 bins, host bins / node ids (uploaded by every call) against DeviceArrays (uploaded once).
WALL time per call (time.perf_counter around the call and a stream synchronisation), which includes what each side must
upload and the host loops of the host-list calls, and for (a) and (b) also the HIP-event time of the stream. Ciphertexts
are random residues mod n^2; (a) gives them exponents 0 .. 2. Both sides must give the same bits, which is asserted. One
warm-up call per side, then --rounds rounds that alternate the sides. Writes profiles/didx_ab.json (--out) after every
case and prints each row.

    python tools/didx_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--bits 1024,2048] [--quick] [--out ...]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_CT, N_SEG, HIST_F, HIST_B = 262144, 512, 16, 32


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def load_parent(path, ref, names):
    """A library of the parent commit: the entry points it has, declared as the current library declares them (it lacks
    the device-index calls, so _native.load_library would refuse it)."""
    plib = ctypes.CDLL(path)
    for name in names:
        try:
            f = getattr(plib, name)
        except AttributeError:
            continue
        f.argtypes, f.restype = getattr(ref, name).argtypes, getattr(ref, name).restype
    return plib


def stats(ms):
    med = statistics.median(ms)
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--quick", action="store_true", help="4096 ciphertexts: a smoke run of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "didx_ab.json"))
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
    n = 4096 if args.quick else N_CT
    result = {"a_kind": "resident lists: pai_segment_add_idx_dev / pai_take_idx_dev / DeviceArray operands, this library",
              "b_kind": "host lists: pai_segment_add_dev / pai_take_dev / numpy operands, "
                        + ("parent library for (a) and (b)" if have_parent else "this library"),
              "time": "wall ms per call including the stream synchronisation; event_ms: HIP events on the stream",
              "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "N": n,
              "sha256": {"library": sha256(N.LIB_PATH)}, "segment_add": [], "take": [], "boosting_level": []}
    if have_parent:
        result["sha256"]["parent"] = sha256(args.parent)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")

    def timed(fn):
        """(wall ms, event ms) of fn and of the stream work it queued."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def ab(run_a, run_b, same, row, where):
        run_a()
        run_b()
        torch.cuda.synchronize()
        wall, ev = {"a": [], "b": []}, {"a": [], "b": []}
        for _ in range(args.rounds):
            for side, fn in (("a", run_a), ("b", run_b)):
                w, e = timed(fn)
                wall[side].append(w)
                ev[side].append(e)
        torch.cuda.synchronize()
        row["identical"] = bool(same())
        assert row["identical"], row
        for side in "ab":
            row[side] = stats(wall[side])
            row[side]["event_ms"] = stats(ev[side])["median_ms"]
        row["speedup_b_over_a"] = round(row["b"]["median_ms"] / row["a"]["median_ms"], 3)
        row["a_faster_beyond_spread"] = bool(max(wall["a"]) < min(wall["b"]))
        row["a_slower_beyond_spread"] = bool(min(wall["a"]) > max(wall["b"]))
        result[where].append(row)
        save()
        print(json.dumps(row), flush=True)

    for nb in (int(v) for v in args.bits.split(",")):
        ctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=lib)
        pctx = N.Context(int(keys[str(nb)]["n"], 16), 0, lib=plib) if have_parent else ctx
        W = ctx.ct_words
        g = torch.Generator(device=dev).manual_seed(nb + n)
        ct = torch.randint(0, 2 ** 31 - 1, (n, W), dtype=torch.int32, device=dev, generator=g)
        ct[:, W - 1] = 0                                       # < 2^(32 (W - 1)) < n^2
        ex = torch.randint(0, 3, (n,), dtype=torch.int32, device=dev, generator=g)
        rng = np.random.default_rng(nb)
        perm = rng.permutation(n).astype(np.int64)
        d_perm = torch.from_numpy(perm).to(dev)
        d_bad = torch.zeros(2, dtype=torch.int64, device=dev)
        s = stream.cuda_stream

        # (a) segment sums
        for nseg in ((N_SEG, n // 4) if not args.quick else (16, n // 4)):
            off = (np.arange(nseg + 1, dtype=np.int64) * (n // nseg))
            d_off = torch.from_numpy(off).to(dev)
            oa = (torch.empty((nseg, W), dtype=torch.int32, device=dev), torch.empty(nseg, dtype=torch.int32, device=dev))
            ob = (torch.empty_like(oa[0]), torch.empty_like(oa[1]))

            def run_a():
                rc = lib.pai_segment_add_idx_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n, d_perm.data_ptr(), n,
                                                 d_off.data_ptr(), nseg, oa[0].data_ptr(), oa[1].data_ptr(), d_bad.data_ptr(), s)
                assert rc == 0, lib.pai_last_error()

            def run_b():
                rc = plib.pai_segment_add_dev(pctx.handle, ct.data_ptr(), ex.data_ptr(), n, perm.ctypes.data, off.ctypes.data,
                                              nseg, ob[0].data_ptr(), ob[1].data_ptr(), s)
                assert rc == 0, plib.pai_last_error()
            ab(run_a, run_b, lambda: torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1]) and bool((d_bad == -1).all()),
               {"nb": nb, "N": n, "nseg": nseg, "members": n // nseg}, "segment_add")

        # (b) take
        ta = (torch.empty((n, W), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        tb = (torch.empty_like(ta[0]), torch.empty_like(ta[1]))

        def take_a():
            rc = lib.pai_take_idx_dev(ctx.handle, ct.data_ptr(), ex.data_ptr(), n, d_perm.data_ptr(), n, 0, ta[0].data_ptr(),
                                      ta[1].data_ptr(), d_bad.data_ptr(), s)
            assert rc == 0, lib.pai_last_error()

        def take_b():
            rc = plib.pai_take_dev(pctx.handle, ct.data_ptr(), ex.data_ptr(), n, perm.ctypes.data, n, tb[0].data_ptr(),
                                   tb[1].data_ptr(), s)
            assert rc == 0, plib.pai_last_error()
        ab(take_a, take_b, lambda: torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1]) and bool((d_bad == -1).all()),
           {"nb": nb, "N": n, "M": n}, "take")
        del ta, tb

        # (c) one boosting level through the Python layer (this library on both sides: the package's own contexts)
        from flex.crypto.paillier.device_buffer import DeviceCiphertextBuffer, device_array
        from flex.crypto.paillier.keypair import PaillierPublicKey
        pk = PaillierPublicKey(int(keys[str(nb)]["n"], 16))
        buf = DeviceCiphertextBuffer.from_pointers(pk, ct.data_ptr(), ex.data_ptr(), n, owner=(ct, ex), device=0)
        bins = rng.integers(0, HIST_B, (n, HIST_F)).astype(np.uint8)
        node = np.zeros(n, dtype=np.int32)
        d_bins, d_node = device_array(bins, 0), device_array(node, 0)
        keep = {}

        def level(b, nd, tag):
            def run():
                hist, _ = buf.histogram(b, HIST_B, node=nd, n_nodes=1)
                keep[tag] = hist.cumsum(axis=2)
            return run
        ab(level(d_bins, d_node, "a"), level(bins, node, "b"),
           lambda: np.array_equal(keep["a"].to_host().words, keep["b"].to_host().words),
           {"nb": nb, "N": n, "F": HIST_F, "B": HIST_B, "bins_bytes": bins.nbytes, "node_bytes": node.nbytes},
           "boosting_level")
        keep.clear()
        del buf, d_bins, d_node, ct, ex, ctx, pctx
    save()


if __name__ == "__main__":
    main()
