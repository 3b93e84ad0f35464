"""The stage-B address pack (kanpyo_amd/csrc/kgpu_tilepack.h: a tile's node and bucket LDS address in one word, computed by the gather and unpacked by
the sweep) on the CPU: tests/c_abi/tile_pack.cpp is built with g++ against the header alone -- that the header needs no HIP is part of the test -- and
checks the round trip of every 8-byte aligned address against the extreme addresses of the other half-word, up to 160 KB of LDS, and that the byte
form refuses the LDS sizes it cannot hold."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "tile_pack.cpp")


def _build(d, extra_src=None):
    exe = os.path.join(d, "tile_pack")
    src = SRC
    if extra_src is not None:
        src = os.path.join(d, "refuse.cpp")
        with open(src, "w") as f:
            f.write(extra_src)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "kanpyo_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_tile_pack_round_trip():
    with tempfile.TemporaryDirectory() as d:
        exe, r = _build(d)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_byte_form_refuses_large_lds_statically():
    """A kernel that picked the byte form for a pool above 64 KB must not compile: the check a launch makes is `fits`, usable in a static_assert."""
    prog = '#include "kgpu_tilepack.h"\nstatic_assert(kgpu::TilePack<%d>::fits(%d), "lds");\nint main() { return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        for shift, lds, ok in ((0, 64 * 1024, True), (0, 80 * 1024, False), (0, 160 * 1024, False), (3, 160 * 1024, True), (3, 1024 * 1024, False)):
            _, r = _build(d, prog % (shift, lds))
            assert (r.returncode == 0) == ok, (shift, lds, r.stderr)
