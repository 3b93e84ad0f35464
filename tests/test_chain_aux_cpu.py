"""Chain::aux_one_launch (kanpyo_amd/csrc/kgpu_chain.cpp) on the CPU, no device: which chains get their scan and compaction as one launch without LDS --
pool-only chains and pool chains without small_scan up to AUX_ONE_LAUNCH_MAX sentences; not windowed chains, not long_share, not tail chains, not
larger batches.  tests/c_abi/chain_aux.cpp is built with g++ against kgpu_chain.cpp alone."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "chain_aux.cpp")
CHAIN = os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_chain.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_chain_aux_one_launch():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chain_aux")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, CHAIN, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = {k: v for k, v in os.environ.items() if not k.startswith("KGPU_")}
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout + r.stderr
