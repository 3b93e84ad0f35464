"""The chunk cutter and the arena step of the chunked host calls (kanpyo_amd/csrc/kgpu_chunk_policy.h: cut_chunk, arena_step) on the CPU, no device:
tests/c_abi/chunk_policy.cpp is built with g++ against the header alone -- that it builds without HIP is part of the test -- and checks both functions
against values written out by hand from the loops the host calls carried before."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "chunk_policy.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_chunk_policy():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chunk_policy")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout + r.stderr
