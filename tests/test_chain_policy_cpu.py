"""The launch-chain policy (kanpyo_amd/csrc/kgpu_chain.cpp: the plan, the chain of a batch, its tail, the feedback from its outcome) on the CPU, no
device: tests/c_abi/chain_policy.cpp is built with g++ against kgpu_chain.cpp alone -- that the module builds without HIP is part of the test -- and
checks the chains and the adaptive rules against the values the runtime computed before the policy had a module of its own."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "chain_policy.cpp")
CHAIN = os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_chain.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_chain_policy():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chain_policy")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, CHAIN, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = {k: v for k, v in os.environ.items() if not k.startswith("KGPU_")}
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "FAIL" not in r.stdout, r.stdout + r.stderr
