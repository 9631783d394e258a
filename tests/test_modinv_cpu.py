"""csrc/modinv_step.hpp on the host: tests/cpu/modinv_check.cpp, built with the address and undefined-behaviour
sanitizers, runs the step routine, row plan, Montgomery coefficient and round count through a plain multi-word loop for
W in {1, 2, 33, 64, 256} over the edge moduli and residues of tests/test_gpu_modinv.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_modinv_rounds_with_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "modinv_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ibond-flex_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "modinv_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert " 0 failures" in run.stdout
