"""A plain bench.py run on the GPU (no --full): one timed step on a small vector, run twice with --dump-outputs.

* the result line holds the headline fields, `steps` timed steps, and in `extra` only what the timed steps themselves
  yield: no leg that is behind --full (decrypt check, generic / public-key paths, fresh keys, nb = 1024, configs[2]/[3],
  host boundary, contention, CPU baseline) has run;
* the two runs write identical .npy files (same inputs, same obfuscators);
* the dumped ciphertexts are the sampler's: rows checked bit for bit against the oracle's restatement.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2053                      # odd, more than one block
STEPS, WARMUP = 1, 1
PLAIN_EXTRA = {"obfuscator_index_bases", "dumped_outputs", "stages", "path", "fixed_base", "encrypt_call_ms",
               "path_int_mac_frac", "hbm_algorithmic_gbs", "w_enc_equivalent"}


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("bench_plain")
    dirs = [str(base / f"run{i}") for i in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                               "--warmup", str(WARMUP), "--n", str(N), "--fb-window", "16", "--dump-outputs", d],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for d in dirs]
    lines = []
    for p in procs:
        out, err = p.communicate(timeout=240)
        assert p.returncode == 0, err[-2000:]
        lines.append(json.loads(out.strip().splitlines()[-1]))
    return lines, dirs


def test_plain_run_reports_only_the_timed_steps(plain_runs):
    lines, _ = plain_runs
    for d in lines:
        assert d["metric"] == "Paillier-2048 encrypts/sec (device-resident), 1M-elem float32 array"
        assert d["unit"] == "encrypts/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
        assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["full"] is False
        assert d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(N * STEPS / (d["ms_per_step"] * STEPS * 1e-3), rel=1e-9)
        assert d["cpu_baseline"] is None
        assert set(d["extra"]) == PLAIN_EXTRA
        assert d["obfuscator_key"].startswith("fixed")
        # the last timed step is step index WARMUP + STEPS - 1: its obfuscators start that many x N past the rank's base
        assert d["extra"]["dumped_outputs"]["obfuscator_index_base"] == (WARMUP + STEPS - 1) * N
        assert d["extra"]["path"].startswith("crt-fixedbase")


def test_two_runs_dump_identical_arrays(plain_runs):
    _, dirs = plain_runs
    names = sorted(os.listdir(dirs[0]))
    assert names == ["ciphertext_words.npy", "exponents.npy", "sample_index.npy"] == sorted(os.listdir(dirs[1]))
    total = 0
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    assert np.load(os.path.join(dirs[0], "ciphertext_words.npy")).shape == (N, 128)
    assert np.array_equal(np.load(os.path.join(dirs[0], "sample_index.npy")), np.arange(N))


def test_dumped_rows_match_the_oracle(plain_runs):
    from flex.crypto.paillier import _native
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    from oracle import paillier_oracle as O
    lines, dirs = plain_runs
    fb = lines[0]["extra"]["fixed_base"]
    info = (fb["g_p"], fb["g_q"], fb["digits"], fb["window_bits"])
    base = lines[0]["extra"]["dumped_outputs"]["obfuscator_index_base"]
    pk, sk = generate_paillier_keypair(2048, seed=1)
    key = O.Key(pk.n, sk.p, sk.q)
    x = np.random.default_rng(0).standard_normal(N, dtype=np.float32)
    rk = hashlib.sha256(b"flexpai-bench-key").digest()
    ct = np.load(os.path.join(dirs[0], "ciphertext_words.npy"))
    ex = np.load(os.path.join(dirs[0], "exponents.npy"))
    assert np.all(ct >= 0) and np.all(ct < 2.0 ** 32) and np.array_equal(ct, np.floor(ct))
    for i in (0, 1, N // 2, N - 1):
        got = (_native.words_to_ints(ct[i:i + 1].astype(np.uint32))[0], int(ex[i]))
        assert got == O.fb_encrypt_value(x[i], key, rk, base + i, info), i
