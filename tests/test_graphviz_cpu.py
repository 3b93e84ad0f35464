"""`kanpyo graphviz` on the device, the parts that need no device: the label pool of the node lines (src/graphviz.rs:56-89: the names
that are not "*", joined with '/') through the host-only kgpu_debug_label_pool hook against a Python join, the command line, the stdin
reader (src/bin/kanpyo.rs:134-143) as a function on bytes, and a strict-C99 consumer of kgpu_graphviz_batch that must compile against the
header and link (tests/test_gpu_graphviz.py runs it)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kanpyo_amd import _lib
from kanpyo_amd.dictfile import MorphFeatureTable


def _label_pool(known: MorphFeatureTable, unk: MorphFeatureTable, n_morphs: int, n_unk: int, cap: int = 4096):
    a, b = np.frombuffer(known.encode(), dtype=np.uint8), np.frombuffer(unk.encode(), dtype=np.uint8)
    off = np.zeros(n_morphs + n_unk + 1, dtype=np.uint32)
    pool = np.zeros(max(cap, 1), dtype=np.uint8)
    got = C.c_uint64(0)
    rc = _lib.lib().kgpu_debug_label_pool(a.ctypes.data, a.size, b.ctypes.data, b.size, n_morphs, n_unk, pool.ctypes.data, cap, off.ctypes.data, C.byref(got))
    return rc, pool[: got.value].tobytes() if rc == _lib.KGPU_OK else b"", off.tolist(), got.value


def _rows(pool, off):
    return [pool[off[i] : off[i + 1]].decode() for i in range(len(off) - 1)]


def _join(rows):
    return ["/".join(f for f in r if f != "*") for r in rows]


def test_label_pool_is_the_python_join():
    known_rows = [
        ["名詞", "*", "一般"],          # '*' in the middle
        ["*", "*", "*"],                # all '*': the empty string
        ["a,b", "c"],                   # a name with ','
        ["x/y", "*", "z"],              # a name with '/'
        ["", "*", "", "q"],             # the empty name is kept
        ["**", "*x", "*"],              # only the name "*" itself is dropped
        [],                             # a row without features
    ]
    unk_rows = [["未知", "*"], ["*"], ["", ""]]
    known, unk = MorphFeatureTable.from_features(known_rows), MorphFeatureTable.from_features(unk_rows)
    rc, pool, off, size = _label_pool(known, unk, len(known_rows), len(unk_rows))
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    want = _join([known.features(i + 1) for i in range(len(known_rows))]) + _join([unk.features(i + 1) for i in range(len(unk_rows))])
    assert _rows(pool, off) == want
    assert want[:5] == ["名詞/一般", "", "a,b/c", "x/y/z", "//q"] and want[-1] == "/"
    assert size == len("".join(want).encode()) and off[0] == 0 and off[-1] == size
    # the same index space as the ','-joined pool: one row per (unknown) morph, rows past the morphs left out
    rc, pool, off, _ = _label_pool(known, unk, 3, 1)
    assert rc == _lib.KGPU_OK and _rows(pool, off) == want[:3] + [want[len(known_rows)]]
    # the size protocol of kgpu_debug_feature_pool
    rc, _, _, need = _label_pool(known, unk, len(known_rows), len(unk_rows), cap=size - 1)
    assert rc == _lib.KGPU_ERR_CAPACITY and need == size


def test_label_pool_validates_as_the_feature_pool_does():
    unk = MorphFeatureTable([[1]], ["", "u"])
    rc, *_ = _label_pool(MorphFeatureTable([[1], [2], [9]], ["", "a", "b"]), unk, 3, 1)   # a feature id past name_list in a nameable row
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:181" in _lib.lib().kgpu_last_error().decode()
    rc, *_ = _label_pool(MorphFeatureTable([[1]], ["", "a"]), MorphFeatureTable([[1], [7]], ["", "u"]), 1, 2)
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:188" in _lib.lib().kgpu_last_error().decode()
    rc, *_ = _label_pool(MorphFeatureTable([[1]], ["", "a"]), unk, 2, 1)                  # fewer rows than morphs
    assert rc == _lib.KGPU_ERR_BAD_DICT
    rc, pool, off, _ = _label_pool(MorphFeatureTable([[1], [2], [9]], ["", "*", "b"]), unk, 2, 1)   # rows past the morphs are not checked
    assert rc == _lib.KGPU_OK and _rows(pool, off) == ["", "b", "u"]
    a = np.frombuffer(b"\x01", dtype=np.uint8)   # a truncated table
    got = C.c_uint64(0)
    off = np.zeros(3, dtype=np.uint32)
    rc = _lib.lib().kgpu_debug_label_pool(a.ctypes.data, a.size, a.ctypes.data, a.size, 1, 1, None, 0, off.ctypes.data, C.byref(got))
    assert rc == _lib.KGPU_ERR_BAD_DICT


def test_command_line():
    from kanpyo_amd import cli

    a = cli.parse_args(["graphviz"])
    assert (a.command, a.input, a.full_state, a.dpi, a.custom_dict, a.dict) == ("graphviz", None, False, 48, None, "ipa")
    a = cli.parse_args(["graphviz", "-f", "--dpi", "300", "-c", "x.dict", "すもも "])
    assert (a.command, a.input, a.full_state, a.dpi, a.custom_dict) == ("graphviz", "すもも ", True, 300, "x.dict")
    a = cli.parse_args(["graphviz", "--full-state", "--custom-dict", "y.dict", "-d", "ipa"])
    assert a.full_state is True and a.custom_dict == "y.dict" and a.input is None
    for bad in ("many", "-1", "18446744073709551616", "4.5", ""):   # --dpi is a usize (src/bin/kanpyo.rs:45-47)
        with pytest.raises(SystemExit):
            cli.parse_args(["graphviz", "--dpi", bad])
    assert cli.parse_args(["graphviz", "--dpi", "18446744073709551615"]).dpi == 2**64 - 1 and cli.parse_args(["graphviz", "--dpi", "+7"]).dpi == 7
    with pytest.raises(SystemExit):
        cli.parse_args(["graphviz", "-f", "1", "2"])   # -f is a flag: two positionals are one too many
    a = cli.parse_args([])   # no subcommand still means tokenize from stdin
    assert a.command == "tokenize" and a.input is None and a.split == "host"
    a = cli.parse_args(["tokenize", "-c", "x.dict", "abc"])
    assert (a.command, a.custom_dict, a.input) == ("tokenize", "x.dict", "abc")


def test_stdin_reader_takes_the_first_line_and_trims_it():
    from kanpyo_amd.cli import first_line

    assert first_line("すもも\nもも\n".encode()) == "すもも".encode()
    assert first_line("すもも \t　\r\nもも".encode()) == "すもも".encode()
    assert first_line(" すもも   ".encode()) == " すもも".encode()   # no newline at all; leading space stays
    assert first_line(b"") == b"" and first_line(b"\n\nabc") == b"" and first_line(b" \x0b\x0c\x85".decode("latin-1").encode()) == b""
    assert first_line(b"a\x1c\x1f\n") == b"a\x1c\x1f"        # U+001C..001F are not White_Space
    assert first_line("a\u200b\n".encode()) == "a\u200b".encode()   # nor is U+200B
    assert first_line(b"ok\n\xff\xfe\n") == b"ok"             # the lines behind the first are never read
    with pytest.raises(UnicodeDecodeError):
        first_line(b"\xff\xfe\nok\n")


def test_graphviz_consumer_is_strict_c99_and_links(tmp_path):
    exe = str(tmp_path / "graphviz_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "graphviz_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    syms = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    used = {w for line in syms.splitlines() for w in line.split() if w.startswith("kgpu_")}
    assert {"kgpu_dict_create", "kgpu_dict_set_features", "kgpu_graphviz_batch"} <= used
    assert "kgpu_graphviz_batch" in _lib.SYMBOLS and hasattr(_lib.lib(), "kgpu_graphviz_batch")
