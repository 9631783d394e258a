#!/usr/bin/env python3
"""One boosting level's way from the party with the public key to the key holder, with and without
PackedCiphertextBuffer.repack(): N = 262 144 samples, F = 16, B = 32, 8 nodes, g / h packed in two 48-bit slots, 2048-bit
key (--bits), resident buffers, one process, one GPU.

    left = hist.cumsum(axis=2)                    # 4 096 ciphertexts of 2 slots (once, outside the timed steps)
    a:  send(left.to_wire(be_secure=True))        # obfuscate 4 096, 4 096 ciphertexts on the wire, 4 096 decryptions
    b:  send(left.repack().to_wire(be_secure=True))   # fold, obfuscate ceil(4 096 / g), as many decryptions

Timed per step, wall time (perf_counter) around the call and a 4-byte download that waits for the device: fold
(repack), obfuscate (apply_obfuscation), wire (to_wire of the obfuscated buffer: the download and the header), decrypt
(from_wire(device=True) + decryptor.decrypt, the range check of the received words included). One warm-up, then --rounds
rounds that alternate a and b; medians. Both sides must decrypt to the same values, which must equal numpy's. Writes
profiles/repack_level.json (--out) and prints it.

    python tools/repack_level.py [--rounds 3] [--samples 262144] [--bits 2048] [--out profiles/repack_level.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ibond-flex_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repack_level.json"))
    args = ap.parse_args()
    from flex.crypto.paillier import _native as N
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.decryptor import PaillierDecryptor
    from flex.crypto.paillier.keypair import PaillierPrivateKey, PaillierPublicKey
    from flex.crypto.paillier.packed_buffer import PackedCiphertextBuffer, PackedLayout
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        k = json.load(f)["keys"][str(args.bits)]
    pk = PaillierPublicKey(int(k["n"], 16))
    sk = PaillierPrivateKey(pk, int(k["p"], 16), int(k["q"], 16))
    dec = PaillierDecryptor(pk, sk)
    S, F, B, NODES = args.samples, 16, 32, 8
    rng = np.random.default_rng(1)
    bins = rng.integers(0, B, (S, F)).astype(np.uint8)
    node = rng.integers(0, NODES, S).astype(np.int32)
    gh = rng.integers(-1000, 1001, (S, 2)).astype(np.int64)
    lay = PackedLayout(pk, 48, 11, 0, 2)
    ctx = _runtime.context(pk, sk)
    # the inputs' obfuscation does not change any later step's work: c0 = 1 + n m, formed on the GPU
    words, st = ctx.encrypt_packed(gh.reshape(-1), lay, N.PAI_OBF_NONE)
    assert not st.any()
    src = PackedCiphertextBuffer(pk, words, lay, 2 * S, (S, 2), True, 1000).to_device()
    hist, cnt = src.histogram(bins, B, node=node, n_nodes=NODES)
    left = hist.cumsum(axis=2)
    want = np.zeros((NODES, F, B, 2), dtype=np.int64)
    for f in range(F):
        np.add.at(want, (node, f, bins[:, f].astype(np.int64)), gh)
    want = np.cumsum(want, axis=2)

    def wait(buf):
        buf.words.mem.download(np.uint32, 1)

    def step(times, name, fn):
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def fresh():
        """A buffer of its own over left's device words, flag cleared. apply_obfuscation sets the flag on the buffer it is
        called on; for resident words it writes into a fresh block (obfuscate_dev), so left's words are only read."""
        return PackedCiphertextBuffer(pk, left.words, left.layout, left.count, left.shape, False, left.bound)

    def side(times, repack):
        buf = fresh()
        if repack:
            def fold():
                out = buf.repack()
                wait(out)
                return out
            buf = step(times, "fold_ms", fold)

        def obf():
            buf.apply_obfuscation()
            wait(buf)
        step(times, "obfuscate_ms", obf)
        wire = step(times, "wire_ms", lambda: buf.to_wire(be_secure=True))
        got = step(times, "decrypt_ms", lambda: dec.decrypt(PackedCiphertextBuffer.from_wire(wire, pk, device=True)))
        return len(wire), int(buf.words.shape[0]), got

    result = {"samples": S, "features": F, "bins": B, "nodes": NODES, "key_bits": args.bits, "rounds": args.rounds,
              "layout": list(lay.as_tuple()), "timing": "wall time (perf_counter) around the step, ended by a download",
              "sides": {}}
    times = {False: {}, True: {}}
    outs = {}
    for rnd in range(args.rounds + 1):                         # round 0 is the warm-up
        for repack in (False, True):
            t = {} if rnd == 0 else times[repack]
            outs[repack] = side(t, repack)
    for repack, name in ((False, "plain"), (True, "repack")):
        nbytes, cts, got = outs[repack]
        row = {"ciphertexts": cts, "wire_bytes": nbytes, "decrypts_to_numpy": bool(np.array_equal(got, want))}
        for key, vals in times[repack].items():
            row[key] = round(statistics.median(vals), 3)
            row[key.replace("_ms", "_repeats_ms")] = [round(v, 3) for v in vals]
        row["total_ms"] = round(sum(statistics.median(v) for v in times[repack].values()), 3)
        result["sides"][name] = row
    result["same_values"] = bool(np.array_equal(outs[False][2], outs[True][2]))
    result["fold_path"] = ctx.fold_path
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
