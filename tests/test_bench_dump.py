"""bench.py --dump-outputs (CPU): the rows kept are a fixed, sorted sample, and the arrays land as float64 .npy files that
hold the 32-bit ciphertext words exactly."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_rows_are_fixed_and_sorted():
    assert np.array_equal(bench.dump_rows(1000), np.arange(1000))
    assert np.array_equal(bench.dump_rows(bench.DUMP_ROWS), np.arange(bench.DUMP_ROWS))
    n = 1 << 20
    a, b = bench.dump_rows(n), bench.dump_rows(n)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert len(a) == bench.DUMP_ROWS and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < n


def test_dump_outputs_writes_exact_float64(tmp_path):
    g = torch.Generator().manual_seed(3)
    n, W = 37, 128
    words = torch.randint(-2 ** 31, 2 ** 31, (n, W), dtype=torch.int64, generator=g).to(torch.int32)
    words[0, 0], words[1, 0] = -1, -2 ** 31            # 0xffffffff and 0x80000000
    exps = torch.randint(-40, 8, (n,), generator=g).to(torch.int32)
    vals = torch.randn(n, dtype=torch.float64, generator=g)
    rows = np.array([0, 1, 5, 36], dtype=np.int64)
    d = str(tmp_path / "out")
    shapes = bench.dump_outputs(d, rows, words, exps, vals)
    assert sorted(os.listdir(d)) == ["ciphertext_words.npy", "exponents.npy", "sample_index.npy", "values.npy"]
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in shapes}
    assert all(v.dtype == np.float64 for v in got.values())
    assert {k: list(v.shape) for k, v in got.items()} == shapes
    assert np.array_equal(got["sample_index"], rows)
    assert np.array_equal(got["ciphertext_words"].astype(np.uint32), words.numpy().view(np.uint32)[rows])
    assert got["ciphertext_words"][0, 0] == 2.0 ** 32 - 1 and got["ciphertext_words"][1, 0] == 2.0 ** 31
    assert np.array_equal(got["exponents"], exps.numpy()[rows])
    assert np.array_equal(got["values"], vals.numpy())


def test_plain_run_turns_every_other_leg_off():
    """The legs behind --full are exactly the --no-* switches of the parser."""
    import re
    with open(os.path.join(ROOT, "bench.py")) as f:
        opts = set(re.findall(r'add_argument\("--no-([a-z0-9-]+)"', f.read()))
    assert opts == {leg.replace("_", "-") for leg in bench.FULL_ONLY_LEGS}
