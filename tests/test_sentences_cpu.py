"""The sentence rule on the host (kgpu_split_sentences_host, kanpyo_amd/csrc/kgpu_sentence_host.cpp over kgpu_sentence_core.h: the scan form, no stack)
against tests/sentence_ref.py (a plain-Python restatement WITH a bracket stack), the hand-derived cases of tests/golden/fixture_sentences.json, the
properties every line must have, the options' and the capacity's checks, and the surface: symbols, argtypes, header, struct layouts, null arguments,
the command line.  No device is needed.  Byte-exact, no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sentence_ref as R
from conftest import ROOT, load_golden
from kanpyo_amd import SENTENCE_DTYPE, _lib, cli, split_sentences_host

INC = os.path.join(ROOT, "include")
# dense in every class: terminators, both kinds of brackets, Space of every width, text, '.', truncated and stray lead and continuation bytes
ALPHABET = [c.encode() for c in R.DEFAULT_TERMINATORS + R.OPENERS + R.CLOSERS + R.SPACES.replace("\n", "") + "あいう漢字abc.．"] + [b"\xe3", b"\x80", b"\xef\xbc", b"\xe2\x80", b"\xc2", b"\x82", b"\xef", b"\xbd"]
SPACE_ENCODINGS = sorted((c.encode() for c in R.SPACES), key=len, reverse=True)


def _host(lines, **kw):
    text, off, rec = split_sentences_host(*R.pack(lines), **kw)
    return text.tobytes(), off.tolist(), [(int(r["line"]), int(r["byte_start"]), int(r["char_start"])) for r in rec]


def _case_lines(c):
    line = bytes.fromhex(c["line_hex"]) if "line_hex" in c else c["line"].encode()
    pieces = [bytes.fromhex(p) for p in c["pieces_hex"]] if "pieces_hex" in c else [p.encode() for p in c["pieces"]]
    return line, pieces, {k: c[k] for k in ("terminators", "brackets") if k in c}


def _random_lines(rng, n_lines, max_parts):
    return [b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=int(rng.integers(0, max_parts + 1)))) for _ in range(n_lines)]


def _only_space(b: bytes) -> bool:
    i = 0
    while i < len(b):
        for e in SPACE_ENCODINGS:
            if b.startswith(e, i):
                i += len(e)
                break
        else:
            return False
    return True


# ---- 1. the examples and the crafted cases --------------------------------------------------------------------------------------------------------
def test_crafted_cases_against_hand_derived_pieces_and_the_restatement():
    cases = load_golden("fixture_sentences.json")["cases"]
    assert len(cases) >= 120
    seen = "".join(c.get("line", "") for c in cases)
    assert all(ch in seen for ch in R.DEFAULT_TERMINATORS + R.OPENERS + R.CLOSERS + R.SPACES.replace("\n", ""))
    assert any(c.get("line") == "。" * 65 for c in cases) and any("line_hex" in c for c in cases)
    for c in cases:
        line, pieces, kw = _case_lines(c)
        text, off, rec = _host([line], **kw)
        assert [text[off[k] : off[k + 1]] for k in range(len(rec))] == pieces, c
        assert (text, off, rec) == R.split_lines([line], **kw), c
    # all of them as one batch: the lines do not see each other
    lines = [_case_lines(c)[0] for c in cases if not _case_lines(c)[2]]
    assert _host(lines) == R.split_lines(lines)
    assert _host([]) == (b"", [0], []) and _host([b""]) == (b"", [0, 0], [(0, 0, 0)])


def test_the_three_examples_of_the_rule():
    for line, pieces in (("彼は「行く。」と言った。次の文！？ 最後", ["彼は「行く。」と言った。", "次の文！？", "最後"]), ("「閉じない。次。", ["「閉じない。", "次。"]),
                         ("閉じ」ない。次（注。）。終", ["閉じ」ない。", "次（注。）。", "終"])):
        text, off, rec = _host([line.encode()])
        assert [text[off[k] : off[k + 1]].decode() for k in range(len(rec))] == pieces


# ---- 2. seeded random lines: the restatement, and the properties of every line ---------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"brackets": False}, {"terminators": ".あ\U0001F600"}], ids=["default", "no_brackets", "custom"])
def test_random_lines_and_their_properties(kw):
    rng = np.random.default_rng(20 + len(kw))
    lines = _random_lines(rng, 1500, 48)
    text, off, rec = _host(lines, **kw)
    assert (text, off, rec) == R.split_lines(lines, **kw)
    by_line = {}
    for k, (li, b, ch) in enumerate(rec):
        by_line.setdefault(li, []).append((b, text[off[k] : off[k + 1]], ch))
    assert sorted(by_line) == list(range(len(lines)))   # every line gives a sentence at least
    again = []
    for li, line in enumerate(lines):
        sents = by_line[li]
        assert sents[0][0] == 0 and sents[-1][0] + len(sents[-1][1]) == len(line), line        # starts at 0, ends at the line's end
        for (b, piece, ch), nxt in zip(sents, sents[1:] + [None]):
            assert line[b : b + len(piece)] == piece and ch == sum(1 for x in line[:b] if x & 0xC0 != 0x80), line
            if nxt is not None:
                gap = line[b + len(piece) : nxt[0]]
                assert _only_space(gap) and len(piece) > 0, line                                   # between two sentences: Space encodings only
            again.append(piece)
    # splitting any sentence again gives that one sentence
    text2, off2, rec2 = _host(again, **kw)
    assert text2 == b"".join(again) and [r[0] for r in rec2] == list(range(len(again))) and all(r[1:] == (0, 0) for r in rec2)


def test_long_lines_and_deep_brackets():
    rng = np.random.default_rng(7)
    lines = _random_lines(rng, 3, 6000) + [b"(" * 70000 + "。".encode() + b")" * 69999 + "。次".encode() + b")" * 5 + "。終".encode()]
    assert _host(lines) == R.split_lines(lines)


# ---- 3. options and capacity ---------------------------------------------------------------------------------------------------------------------------
def test_option_validation():
    utf8, offs = R.pack(["あ。い".encode()])

    def rc_of(o):
        out, ooff, rec, n = np.zeros(16, np.uint8), np.zeros(8, np.uint64), np.zeros(4, SENTENCE_DTYPE), C.c_uint64()
        return _lib.lib().kgpu_split_sentences_host(utf8.ctypes.data, offs.ctypes.data, 1, C.byref(o) if o is not None else None, out.ctypes.data, ooff.ctypes.data,
                                                    rec.ctypes.data, 4, C.byref(n)), n.value

    assert rc_of(None) == (_lib.KGPU_OK, 2) and rc_of(_lib.sentence_opts()) == (_lib.KGPU_OK, 2)
    for bad in (0x20, 0x0A, 0x00, 0x3000, 0xA0, 0x85, 0x2003, ord("("), ord("「"), ord("｣"), ord("】"), 0xD800, 0xDFFF, 0x110000, 0xFFFFFFFF):
        assert rc_of(_lib.sentence_opts([ord("。"), bad]))[0] == _lib.KGPU_ERR_INVALID_ARG, hex(bad)
    for good in (0x21, ord("."), 0x3002, 0x10FFFF, 0x1F600, 0xFF0E, 0x7F, 0x80, 0x7FF, 0x800):
        assert rc_of(_lib.sentence_opts([good]))[0] == _lib.KGPU_OK, hex(good)
    o = _lib.sentence_opts()
    o.flags = 2
    assert rc_of(o)[0] == _lib.KGPU_ERR_INVALID_ARG
    for k in (0, 1):
        o = _lib.sentence_opts()
        o.reserved[k] = 1
        assert rc_of(o)[0] == _lib.KGPU_ERR_INVALID_ARG
    o = _lib.sentence_opts("。")
    o.n_terminators = 17
    assert rc_of(o)[0] == _lib.KGPU_ERR_INVALID_ARG
    assert rc_of(_lib.sentence_opts("。" * 16))[0] == _lib.KGPU_OK
    with pytest.raises(ValueError):
        _lib.sentence_opts("。" * 17)
    with pytest.raises(ValueError):
        _lib.sentence_opts("")
    with pytest.raises(_lib.KgpuError):
        split_sentences_host(utf8, offs, terminators=" ")


def test_capacity_reports_the_exact_count_and_writes_nothing():
    lines = ["あ。い！う？え".encode(), b"", "「お。」か。".encode()]
    utf8, offs = R.pack(lines)
    want = len(R.split_lines(lines)[2])
    assert want == 6
    L = _lib.lib()
    for cap in (0, want - 1):
        out, ooff, rec, n = np.full(64, 0xAB, np.uint8), np.full(16, 0xABAB, np.uint64), np.full(16, 0xAB, np.uint8), C.c_uint64()
        rc = L.kgpu_split_sentences_host(utf8.ctypes.data, offs.ctypes.data, 3, None, out.ctypes.data, ooff.ctypes.data, rec.ctypes.data if cap else None, cap, C.byref(n))
        assert rc == _lib.KGPU_ERR_CAPACITY and n.value == want
        assert (out == 0xAB).all() and (ooff == 0xABAB).all() and (rec == 0xAB).all()
    n = C.c_uint64()
    assert L.kgpu_split_sentences_host(utf8.ctypes.data, offs.ctypes.data, 3, None, None, np.zeros(1, np.uint64).ctypes.data, None, 0, C.byref(n)) == _lib.KGPU_ERR_CAPACITY and n.value == want
    back = np.array([0, 5, 3, 9], dtype=np.uint64)
    assert L.kgpu_split_sentences_host(utf8.ctypes.data, back.ctypes.data, 3, None, None, np.zeros(1, np.uint64).ctypes.data, None, 0, C.byref(n)) == _lib.KGPU_ERR_INVALID_ARG


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_argtypes_header_and_makefile():
    L = _lib.lib()
    header = open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8").read()
    for s, nargs in (("kgpu_split_sentences_host", 9), ("kgpu_split_sentences_batch", 10), ("kgpu_split_sentences_device", 10), ("kgpu_ctx_sync_sentences", 3)):
        assert s in _lib.SYMBOLS and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs and s + "(" in header, s
    assert "---- sentences:" in header and "#define KGPU_SENTENCES_NO_BRACKETS 1u" in header and _lib.KGPU_SENTENCES_NO_BRACKETS == 1
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_sentence.hip") == 2 and "kgpu_sentence_host.cpp" in mk and "kgpu_sentence_batch.cpp" in mk and "kgpu_sentence_core.h" in mk
    import kanpyo_amd
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import Tokenizer

    assert "split_sentences_host" in kanpyo_amd.__all__ and callable(Tokenizer.split_sentences) and callable(Tokenizer.split_sentences_packed)
    assert all(callable(getattr(DeviceContext, m)) for m in ("split_sentences", "sync_sentences", "try_sync_sentences"))


def test_struct_layouts_in_strict_c99(tmp_path):
    src = tmp_path / "sentence_layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "kanpyo_gpu.h"
int main(void) {
    printf("%d %d %d %d ", (int)sizeof(kgpu_sentence), (int)offsetof(kgpu_sentence, line), (int)offsetof(kgpu_sentence, byte_start), (int)offsetof(kgpu_sentence, char_start));
    printf("%d %d %d %d %d\\n", (int)sizeof(kgpu_sentence_opts), (int)offsetof(kgpu_sentence_opts, flags), (int)offsetof(kgpu_sentence_opts, n_terminators),
           (int)offsetof(kgpu_sentence_opts, terminators), (int)offsetof(kgpu_sentence_opts, reserved));
    return 0;
}
""")
    exe = str(tmp_path / "sentence_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 8, 12, 80, 0, 4, 8, 72]
    S, O = _lib.Sentence, _lib.SentenceOpts
    assert [C.sizeof(S), S.line.offset, S.byte_start.offset, S.char_start.offset, C.sizeof(O), O.flags.offset, O.n_terminators.offset, O.terminators.offset, O.reserved.offset] == got
    assert SENTENCE_DTYPE.itemsize == 16 and [SENTENCE_DTYPE.fields[f][1] for f in ("line", "byte_start", "char_start")] == [0, 8, 12]
    assert C.sizeof(R.SentenceOpts) == 80


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    n = C.c_uint64()
    one = np.zeros(2, np.uint64)
    assert L.kgpu_split_sentences_device(None, None, one.ctypes.data, 0, 0, None, None, one.ctypes.data, None, 0) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_ctx_sync_sentences(None, C.byref(n), C.byref(n)) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_split_sentences_batch(None, None, one.ctypes.data, 0, None, None, one.ctypes.data, None, 0, C.byref(n)) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_split_sentences_host(None, None, 0, None, None, one.ctypes.data, None, 0, C.byref(n)) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_split_sentences_host(None, one.ctypes.data, 0, None, None, None, None, 0, C.byref(n)) == _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_split_sentences_host(None, one.ctypes.data, 0, None, None, one.ctypes.data, None, 0, None) == _lib.KGPU_ERR_INVALID_ARG


def test_host_function_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/c_abi/sentence_sanitize.cpp, its own main) linked with kgpu_sentence_host.cpp alone: nothing is loaded into Python."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):   # (the probe of tests/test_prob_cpu.py, before any work)
        pytest.skip("no libasan in this toolchain")
    exe = str(tmp_path / "sentence_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", INC,
                        os.path.join(ROOT, "tests", "c_abi", "sentence_sanitize.cpp"), os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_sentence_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sentence sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_cli_options_and_what_they_do_not_go_with(capsys):
    for cmd in ("tokenize", "wakati", "count", "normalize"):
        a = cli.parse_args([cmd, "--sentences", "--terminators", "。.", "--no-brackets"])
        assert (a.sentences, a.terminators, a.no_brackets) == (True, "。.", True), cmd
        assert cli.parse_args([cmd]).sentences is False
    assert cli.parse_args(["encode", "--vocab", "v.txt", "--sentences"]).sentences is True
    for ok in (["--sentences", "--nbest", "3"], ["--sentences", "--marginal"], ["--sentences", "--sample", "2"], ["--sentences", "--mode", "search"],
               ["--sentences", "--normalize", "nfkc"]):
        assert cli.parse_args(["tokenize"] + ok).sentences is True
    bad = [["tokenize", "--sentences", "--split", "device"], ["wakati", "--terminators", "。"], ["count", "--no-brackets"], ["align", "--sentences"],
           ["graphviz", "--sentences"], ["decode", "--vocab", "v", "--sentences"], ["tokenize", "--sentences", "--terminators", ""],
           ["tokenize", "--sentences", "--terminators", "。" * 17], ["encode", "--vocab", "v", "--sentences", "--offsets"],
           ["encode", "--vocab", "v", "--bos", "a", "--eos", "b", "--sentences", "--max-length", "8", "--pair"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    for cmd in ("tokenize", "wakati", "count", "encode", "normalize"):
        with pytest.raises(SystemExit):
            cli.parse_args([cmd, "--help"])
        text = capsys.readouterr().out
        assert "--sentences" in text and "--terminators" in text and "--no-brackets" in text, cmd
