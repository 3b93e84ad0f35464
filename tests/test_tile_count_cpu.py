"""The stage-B tile count (kanpyo_amd/csrc/kgpu_tilepack.h: tile_count(T, P) = P ? ceil(T / 8) * ceil(P / 8) : 0 -- what the pool kernel's scan reserves
for a start position and what its list builder then writes) on the CPU: tests/c_abi/tile_count.cpp is built with g++ against the header alone and checks
it against counts made the long way for T, P in 0..40, a position nothing ends at (P = 0) having no tile."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "tile_count.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tile_count_against_brute_force():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tile_count")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "kanpyo_amd", "csrc"), SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("ok 1681 shapes") and "FAIL" not in r.stdout, r.stdout + r.stderr
