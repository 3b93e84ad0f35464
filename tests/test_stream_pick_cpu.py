"""pick_stream (kanpyo_amd/csrc/kgpu_chain.cpp) on the CPU, no device: a batch goes to the least-loaded of the dictionary's shared streams, load counted in
bytes.  Equal weights rotate strictly over 3 and 4 streams; eight contexts driven as bench_engine.GpuEngine drives them load three streams 8 / 8 / 8 over any
24 picks and never more than 3 of the batches in flight on one; a 1696-sentence batch among batches of 4096 goes where the bytes say; a single stream, a
wrapping cursor and a load that returns to zero.  tests/c_abi/stream_pick.cpp is built with g++ against kgpu_chain.cpp alone."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "stream_pick.cpp")
CHAIN = os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_chain.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stream_pick():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stream_pick")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, CHAIN, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = {k: v for k, v in os.environ.items() if not k.startswith("KGPU_")}
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout + r.stderr
