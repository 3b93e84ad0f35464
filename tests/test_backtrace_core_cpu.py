"""The pool kernel's backtrace over quads (kanpyo_amd/csrc/kgpu_backtrace_core.h: a node's best predecessor doubled into its four nearest ancestors, the
chase that reads four path nodes a round, where it ends and what K becomes) on the CPU: tests/c_abi/backtrace_core.cpp (its own main) is built by plain g++
against the header alone -- that the header needs no HIP is part of the test -- with the address and undefined-behaviour sanitizers linked statically, and run
as a program.  It makes the two passes as the kernel does (four nodes per lane and trip, clamped lanes, a hop from "none" reading entry N) over random
predecessor forests with N from 1 to 600 -- indices falling strictly along a chain, roots, dead nodes -- and asserts for EVERY start node that the quad
chase gives the plain one-step chase's path and K, with C on both sides of the chain's length, every array a heap block of the size the kernel's carve has."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kanpyo_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c_abi", "backtrace_core.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_quad_chase_against_one_step_chase_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "backtrace_core")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes are linked statically)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_kernel_goes_through_the_header():
    """the kernel's passes and its count of K are the header's functions, not a second spelling of them"""
    src = open(os.path.join(CSRC, "kgpu_pool.hip"), encoding="utf-8").read()
    assert '#include "kgpu_backtrace_core.h"' in src
    for name in ("bt_hop(", "bt_p2(", "bt_path_count("):
        assert name in src, name
    assert "kgpu_backtrace_core.h" in open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()   # a change to it rebuilds the kernel
