#!/usr/bin/env python3
"""A/B of device-resident ciphertext buffers against the host-buffer entry points, in one process on one GPU:

  a  = the chain on a DeviceCiphertextBuffer (device_buffer.py) uploaded before the timed region: what a level of a
       boosting tree costs once the encrypted g / h are resident;
  a1 = a plus the one to_device(): the first level;
  b  = the same chain through the host-buffer entry points of a library built from the PARENT commit (--parent), loaded
       next to this one as tools/mm_ab.py does, called in CiphertextBuffer's order with numpy in and numpy out.

Shapes, at 1024 and 2048 bits, random residues at exponent 0:
  1. a boosting level: N = 262 144 samples, F = 16, B = 32, 8 nodes; histogram -> cumsum(axis=2) -> the cells on the host;
  2. the same chain with g / h packed in two slots of one ciphertext per sample (PackedCiphertextBuffer.to_device());
     side b takes the cell counts on the host first, as the host class does for its slot bound ("host_count_ms"); the
     resident class skips that count where its bound times all samples fits the slot, as here, so most of this shape's
     b / a is that numpy count, not PCIe;
  3. the LR gradient (4096,) @ (4096, 64) -> the 64 results on the host;
  4. to_device() and to_host() of 262 144 ciphertexts in GB/s, next to a plain hipMemcpy of the same bytes from and to
     pinned memory, timed in this tool.
One warm-up per side, then --rounds rounds that alternate the sides. A figure is the WALL time around the call, which ends
with a download or is synchronous: side b's copies are host work that device events would not see. Medians and the spread
(min, max) of the repeats are recorded, whether all sides gave identical outputs, whether every repeat of a lies below
every repeat of b, and the number of levels k from which a1 + (k - 1) a < k b. Writes --out and prints the same JSON.

    python tools/resident_ab.py [--parent ab/libflexpai_parent.so] [--rounds 3] [--samples 262144] [--bits 1024,2048]
                                [--out profiles/resident_ab.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]


def residues(N, W, seed):
    """[N, W] words below 2^(32 (W - 1)) < n^2."""
    words = np.random.default_rng(seed).integers(0, 1 << 32, (N, W), dtype=np.uint64).astype(np.uint32)
    words[:, W - 1] = 0
    return words


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(sides, rounds):
    """{name: ms list} over `rounds` alternating rounds after one warm-up per side, and the last output of each side."""
    outs = {k: fn() for k, fn in sides.items()}
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms, outs[k] = wall(fn)
            times[k].append(ms)
    return times, outs


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats_ms": ms}


def same(x, y):
    return all(np.array_equal(u, v) for u, v in zip(x, y))


def summary(times, outs):
    a, a1, b = times["a"], times["a1"], times["b"]
    ma, ma1, mb = (statistics.median(t) for t in (a, a1, b))
    res = {k: stats(v) for k, v in times.items()}
    res["outputs_identical"] = bool(same(outs["a"], outs["b"]) and same(outs["a1"], outs["b"]))
    res["every_a_below_every_b"] = bool(max(a) < min(b))
    res["b_over_a"] = mb / ma
    res["levels_to_break_even"] = (int((ma1 - ma) // (mb - ma)) + 1 if ma1 > mb else 1) if mb > ma else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "libflexpai_parent.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--bits", default="1024,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_ab.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer, histogram_cells
    from flex.crypto.paillier.keypair import PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    if not os.path.exists(args.parent):
        sys.exit(f"{args.parent}: build the parent commit's libflexpai.so there first (side b)")
    lib_b = N.load_library(args.parent)
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        keys = json.load(f)["keys"]
    S, F, B, NODES = args.samples, 16, 32, 8
    rng = np.random.default_rng(1)
    bins = rng.integers(0, B, (S, F)).astype(np.uint8)
    node = rng.integers(0, NODES, S).astype(np.int32)
    result = {"rounds": args.rounds, "samples": S, "features": F, "bins": B, "nodes": NODES,
              "timing": "wall time around the call (perf_counter), ended by a download or a synchronous entry point",
              "side_b": "host-buffer entry points of the parent commit's library", "keys": {},
              "not_measured": ["4096-bit keys", "mixed exponents", "sparse bins"]}
    # the HIP runtime the library itself runs on, for the plain pinned copies of shape 4
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    for nb in (int(v) for v in args.bits.split(",")):
        pk = PaillierPublicKey(int(keys[str(nb)]["n"], 16))
        cb = N.Context(pk.n, 0, lib=lib_b)
        W = cb.ct_words
        words, exps = residues(S, W, nb), np.zeros(S, dtype=np.int32)
        host = CiphertextBuffer(pk, words, exps, 0, (S,))
        res = {"ct_words": W, "ciphertext_bytes": int(words.nbytes)}

        # 1. a boosting level
        def level_b():
            out, oe, cnt = cb.histogram(words, exps, bins, B, node, NODES)
            out, oe = cb.cumsum(out, np.where(cnt == 0, 0, oe).astype(np.int32), NODES * F, B, 1)
            return out, oe, cnt

        def level_a(dev):
            hist, cnt = dev.histogram(bins, B, node=node, n_nodes=NODES)
            left = hist.cumsum(axis=2).to_host()
            return left.words, left.exps, cnt.reshape(-1)

        resident = host.to_device()
        t, o = measure({"a": lambda: level_a(resident), "a1": lambda: level_a(host.to_device()), "b": level_b}, args.rounds)
        res["boosting_level"] = summary(t, o)

        # 2. the same with g / h in two slots
        lay = PackedLayout(pk, 32, 2, 0, 2)
        packed = PackedCiphertextBuffer(pk, words, lay, 2 * S, (S, 2), False, 1)
        uniform = np.zeros(S, dtype=np.int32)

        def packed_b():
            # the host PackedCiphertextBuffer.histogram takes the counts on the host first, for the slot bound it checks
            # before any GPU call; the resident one (side a) skips them at this bound
            cell = histogram_cells(bins, B, node, NODES)
            bound = int(np.bincount(cell[cell >= 0], minlength=NODES * F * B).max())
            assert bound <= lay.slot_max
            out, _, cnt = cb.histogram(words, uniform, bins, B, node, NODES)
            out, _ = cb.cumsum(out, np.zeros(cnt.size, dtype=np.int32), NODES * F, B, 1)
            return out, cnt

        def packed_a(dev):
            hist, cnt = dev.histogram(bins, B, node=node, n_nodes=NODES)
            return hist.cumsum(axis=2).to_host().words, cnt.reshape(-1)

        packed_dev = packed.to_device()
        t, o = measure({"a": lambda: packed_a(packed_dev), "a1": lambda: packed_a(packed.to_device()), "b": packed_b},
                       args.rounds)
        res["boosting_level_packed"] = summary(t, o)
        res["boosting_level_packed"]["host_count_ms"] = statistics.median(
            wall(lambda: np.bincount(histogram_cells(bins, B, node, NODES).reshape(-1), minlength=NODES * F * B))[0]
            for _ in range(3))
        del packed_dev

        # 3. the LR gradient
        K, d = 4096, 64
        x = rng.standard_normal((K, d))
        small = CiphertextBuffer(pk, words[:K], exps[:K], 0, (K,))
        sres = small.to_device()

        def lr_a(dev):
            g = (dev @ x).to_host()
            return g.words, g.exps

        t, o = measure({"a": lambda: lr_a(sres), "a1": lambda: lr_a(small.to_device()),
                        "b": lambda: cb.matmul(words[:K], exps[:K], 1, K, x.reshape(-1), d)}, args.rounds)
        res["lr_gradient"] = summary(t, o)

        # 4. the transfers, next to a plain pinned hipMemcpy of the same bytes
        nbytes = words.nbytes
        pin = ctypes.c_void_p()
        assert hip.hipHostMalloc(ctypes.byref(pin), ctypes.c_size_t(nbytes), 0) == 0
        ctypes.memmove(pin, words.ctypes.data, nbytes)
        block = N.DeviceMem(nbytes, 0)

        def copy(dst, src, kind):
            assert hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes), kind) == 0
            assert hip.hipDeviceSynchronize() == 0

        t, _ = measure({"to_device": lambda: host.to_device(), "to_host": lambda: resident.to_host(),
                        "pinned_h2d": lambda: copy(block.ptr, pin.value, 1),
                        "pinned_d2h": lambda: copy(pin.value, block.ptr, 2)}, args.rounds)
        res["transfer"] = {k: dict(stats(v), GB_per_s=nbytes / statistics.median(v) / 1e6) for k, v in t.items()}
        hip.hipHostFree(pin)
        result["keys"][str(nb)] = res
        del resident, sres, block
        cb.close()
    result["contexts_a"] = [c.key_bits for c in _runtime.cached_contexts()]
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
