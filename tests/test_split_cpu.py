"""The device form of read_line + trim_end (kgpu_split_lines_device, kgpu_ctx_sync_split) and kgpu_tokenize_text_lines, as far as they go
without a device: the symbols, their declarations, the argument checks that return before anything touches a device, the CLI's option."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from kanpyo_amd import _lib

NAMES = ("kgpu_split_lines_device", "kgpu_ctx_sync_split", "kgpu_tokenize_text_lines")


def test_symbols_are_exported_and_listed():
    L = _lib.lib()
    for s in NAMES:
        assert s in _lib.SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).argtypes, s


def test_header_declares_them_and_is_strict_c99(tmp_path):
    with open(os.path.join(ROOT, "include", "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    for s in NAMES:
        assert f"int {s}(" in header, s
    src = tmp_path / "includer.c"
    src.write_text('#include "kanpyo_gpu.h"\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_null_arguments_are_rejected_without_a_device():
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint8)
    offs = np.zeros(8, dtype=np.uint64)
    n, b = C.c_uint64(7), C.c_uint64(7)
    assert L.kgpu_split_lines_device(None, buf.ctypes.data, 8, buf.ctypes.data + 32, offs.ctypes.data, 8) == _lib.KGPU_ERR_INVALID_ARG
    assert "kgpu_split_lines_device" in L.kgpu_last_error().decode()
    assert L.kgpu_split_lines_device(None, None, 0, None, None, 0) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_ctx_sync_split(None, C.byref(n), C.byref(b)) == _lib.KGPU_ERR_INVALID_ARG
    assert "kgpu_ctx_sync_split" in L.kgpu_last_error().decode()
    assert L.kgpu_ctx_sync_split(None, None, None) == _lib.KGPU_ERR_INVALID_ARG
    text = np.frombuffer(b"a\nb\n", dtype=np.uint8)
    args = (text.ctypes.data, text.size, buf.ctypes.data, buf.size, offs.ctypes.data, offs.size, None)
    assert L.kgpu_tokenize_text_lines(None, *args, C.byref(n), C.byref(b)) == _lib.KGPU_ERR_INVALID_ARG
    assert "kgpu_tokenize_text_lines" in L.kgpu_last_error().decode()
    assert L.kgpu_tokenize_text_lines(None, None, 1 << 32, None, 0, None, 0, None, None, None) == _lib.KGPU_ERR_INVALID_ARG


def test_cli_help_lists_the_split_option():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "--help"], capture_output=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    out = r.stdout.decode()
    assert "--split {host,device}" in out and "default: host" in out
