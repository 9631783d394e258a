"""The digit cut of the fixed-base exponent (csrc/fb_cut.hpp) on the host: tests/cpu/fb_cut_check.cpp, built with the
address and undefined-behaviour sanitizers, walks kb in {512, 1024, 1023, 1025} x asked windows {8, 12, 16, 22, 23, 24}
x budgets one byte below, at and above every threshold at which a plan can change, and asserts for each: the widths sum
to at least kb, none exceeds 24 or the asked window, the tables fit the budget, the digit count is minimal, the plan is
exactly the uniform plan whenever no digit is saved, and digits cut at the plan's offsets reassemble to a_h."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fb_cut_planner_with_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fb_cut_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ibond-flex_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "fb_cut_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout
