"""Text normalisation without a device (include/kanpyo_gpu.h, "text normalisation"): the host function kgpu_normalize_host -- the definition of every
device result -- against tests/golden/fixture_normalize.json and against Python's unicodedata, exhaustively over the scalar values and the
composition pairs and on seeded random strings; the committed tables against a fresh run of their generator; the host module alone under
AddressSanitizer + UBSan; the new symbols, the header, the argument errors, the CLI's options, and the binding's normalize= keyword over a stub
library (normalize=None reaches no normalise entry point)."""
import ctypes as C
import gc
import os
import subprocess
import unicodedata

import numpy as np
import pytest

import normalize_ref as N
from conftest import ROOT
from kanpyo_amd import _lib
from normalize_cases import StubLib, same_unicode

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "kanpyo_amd", "csrc")
NEW = ("kgpu_normalize_unicode_version", "kgpu_normalize_host", "kgpu_normalize_batch", "kgpu_normalize_text", "kgpu_normalize_device", "kgpu_ctx_sync_normalize")
SAME_UNICODE = same_unicode()


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_listed_cases():
    g, cases = N.fixture_cases()
    names = {name for name, *_ in cases}
    assert g["max_segment"] == _lib.KGPU_NORMALIZE_MAX_SEGMENT == 64 and len(cases) >= 70
    for want in ("ascii", "japanese", "empty", "mixed", "ka_dakuten_across_16", "ka_dakuten_across_64", "e_dot_acute", "e_acute_dot", "u0344", "u0f73", "u1e9b_u0323",
                 "ufdfa", "hangul_l_v_t", "hangul_lv_t", "hangul_lvt_v", "ohm_angstrom", "cjk_compat", "bengali", "leading_mark", "marks_63", "marks_64", "marks_65",
                 "invalid_truncated", "invalid_overlong", "invalid_surrogate", "invalid_ff"):
        assert want in names, want
    by = {name: (raw, exp) for name, raw, exp in cases}
    assert by["mixed"][0].decode() == "ﾊﾝｶｸｶﾀｶﾅﾃﾞｽ｡ＡＢＣ１２３㈱①ｶﾞｷﾞｸﾞ　東京" and by["mixed"][1]["NFKC"][0].decode() == "ハンカクカタカナデス。ABC123(株)1ガギグ 東京"
    assert by["mixed"][1]["NFC"][0] == by["mixed"][0]
    assert by["marks_64"][1]["NFKC"][1] == 0 and by["marks_65"][1]["NFKC"] == (by["marks_65"][0], 4) and by["marks_63"][1]["NFC"][1] == 0
    assert by["ufdfa"][1]["NFKC"][0] == unicodedata.normalize("NFKC", "ﷺ").encode() and len(by["ufdfa"][1]["NFKC"][0]) == 33
    assert by["hangul_l_v_t"][1]["NFC"][0] == "각".encode() and by["hangul_lvt_v"][1]["NFC"][0] == "각ᅡ".encode()
    assert by["e_acute_dot"][1]["NFC"][0] == by["e_dot_acute"][1]["NFC"][0] == "ẹ́".encode()
    assert all(exp[f] == (raw, 1) for name, raw, exp in cases if name.startswith("invalid_") for f in N.FORMS)


def test_host_function_reproduces_the_fixture():
    _, cases = N.fixture_cases()
    for name, raw, exp in cases:
        for form, (want, status) in exp.items():
            assert N.host(raw, form) == (0, want, len(want), status), (name, form)


@SAME_UNICODE
def test_fixture_is_what_unicodedata_gives():
    _, cases = N.fixture_cases()
    for name, raw, exp in cases:
        for form, (want, status) in exp.items():
            assert N.GEN.normalize_line(raw, form) == (want, status), (name, form)
            if status == 0:
                assert want == unicodedata.normalize(form, raw.decode()).encode(), (name, form)


def test_capacity_protocol_of_the_host_function():
    raw = "ｶﾞＡﷺ".encode()
    want = unicodedata.normalize("NFKC", raw.decode()).encode() if N.versions_agree() else N.host(raw, "NFKC")[1]
    assert N.host(raw, "NFKC", 0) == (_lib.KGPU_ERR_CAPACITY, b"", len(want), 0)
    assert N.host(raw, "NFKC", len(want) - 1) == (_lib.KGPU_ERR_CAPACITY, b"", len(want), 0)
    assert N.host(raw, "NFKC", len(want)) == (0, want, len(want), 0)
    assert N.host(b"", "NFC", 0) == (0, b"", 0, 0)
    assert N.host(b"\xff", "NFC", 0) == (_lib.KGPU_ERR_CAPACITY, b"", 1, 1)   # an invalid line is copied: it needs its own length


# ---- against unicodedata ----------------------------------------------------------------------------------------------------------------------
def _batch_host(strings, form):
    """Many strings through kgpu_normalize_host with one pair of buffers (the exhaustive run makes millions of calls)."""
    L = _lib.lib()
    out = np.empty(4096, dtype=np.uint8)
    got, st = C.c_uint64(0), C.c_uint8(0)
    fn, f, optr = L.kgpu_normalize_host, N.FORMS[form], out.ctypes.data
    res = []
    for s in strings:
        b = s.encode("utf-8")
        assert fn(f, b, len(b), optr, 4096, C.byref(got), C.byref(st)) == 0 and st.value == 0, (s, form)
        res.append(out[: got.value].tobytes())
    return res


@SAME_UNICODE
@pytest.mark.parametrize("form", list(N.FORMS))
def test_every_scalar_value(form):
    """All 1 112 064 scalar values, each a line of its own."""
    norm = unicodedata.normalize
    for lo in range(0, 0x110000, 0x8000):
        chars = [chr(cp) for cp in range(lo, lo + 0x8000) if not 0xD800 <= cp <= 0xDFFF]
        got = _batch_host(chars, form)
        want = [norm(form, c).encode("utf-8") for c in chars]
        if got != want:
            bad = [hex(ord(c)) for c, g, w in zip(chars, got, want) if g != w]
            pytest.fail(f"{form}: {len(bad)} code points differ, first {bad[:8]}")


@SAME_UNICODE
@pytest.mark.parametrize("form", list(N.FORMS))
def test_every_composition_pair(form):
    pairs, seconds = N.GEN.pairs_and_seconds()
    assert len(pairs) == 941 or unicodedata.unidata_version != "13.0.0"
    strings = [chr(a) + chr(b) for a, b in pairs] + ["a" + chr(a) + chr(b) for a, b in pairs] + [chr(c) for c in pairs.values()]
    assert _batch_host(strings, form) == [unicodedata.normalize(form, s).encode() for s in strings]


@SAME_UNICODE
@pytest.mark.parametrize("form", list(N.FORMS))
def test_random_strings(form):
    strings = N.random_strings(20260101, 30000)
    got = _batch_host(strings, form)
    want = [unicodedata.normalize(form, s).encode() for s in strings]
    bad = [s for s, g, w in zip(strings, got, want) if g != w]
    assert not bad, [[hex(ord(c)) for c in s] for s in bad[:5]]
    assert sum(g != s.encode() for s, g in zip(strings, got)) > 10000   # (the pool is awkward: most strings change)


@SAME_UNICODE
def test_boundary_definition_matches_the_tables():
    """The property word's boundary and inert bits are the header's definition, and a segment of one inert code point is a fixed point."""
    gen = N.GEN
    for form in N.FORMS:
        for cp in N.AWKWARD + list(range(0x3040, 0x3100)) + list(range(0xFF00, 0xFFF0)):
            ch = chr(cp)
            b = gen.boundary_before(cp, form)
            if b and unicodedata.normalize(form, ch) == ch:   # inert: copied as it is, between any neighbours that are boundaries
                assert N.host(("x" + ch + "y").encode(), form)[1] == ("x" + ch + "y").encode()
    assert gen.boundary_before(ord("Ａ"), "NFKC") and gen.boundary_before(ord("ｶ"), "NFKC") and not gen.boundary_before(ord("ﾞ"), "NFKC")
    assert [len(s) for s in gen.segments("ＡＢＣ", "NFKC")] == [1, 1, 1] and list(gen.segments("ｶﾞ", "NFKC")) == ["ｶﾞ"]
    assert not gen.boundary_before(0x1161, "NFC") and not gen.boundary_before(0x11A8, "NFC") and not gen.boundary_before(0x09BE, "NFC") and gen.boundary_before(0xAC00, "NFC")


# ---- the generated file ---------------------------------------------------------------------------------------------------------------------------
@SAME_UNICODE
def test_generator_reproduces_the_committed_tables_and_fixture(tmp_path):
    N.GEN.main(["--out", str(tmp_path)])
    with open(tmp_path / "kgpu_normalize_data.inc", "rb") as f, open(os.path.join(CSRC, "kgpu_normalize_data.inc"), "rb") as g:
        assert f.read() == g.read(), "kgpu_normalize_data.inc is not what tools/gen_normalize_tables.py writes"
    with open(os.path.join(ROOT, "tests", "golden", "fixture_normalize.json"), encoding="ascii") as g:
        assert N.GEN.render_fixture() == g.read()


def test_generated_file_is_not_built_from_and_stays_small():
    with open(os.path.join(CSRC, "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert "gen_normalize_tables" not in mk and "kgpu_normalize.hip" in mk and "kgpu_normalize_host.cpp" in mk and "kgpu_normalize_table.cpp" in mk
    assert mk.count("kgpu_normalize.hip") == 2   # SRCS and the resource-usage target
    assert os.path.getsize(os.path.join(CSRC, "kgpu_normalize_data.inc")) < (1 << 20)
    with open(os.path.join(CSRC, "kgpu_normalize_table.cpp"), encoding="utf-8") as f:
        assert "hip" not in f.read().lower().replace("hip-free", "").replace("kgpu_normalize.hip", "")


# ---- the host module alone, under the sanitizers ----------------------------------------------------------------------------------------------------
def test_host_module_alone_under_asan_ubsan(tmp_path):
    """kgpu_normalize_table.cpp and tests/c_abi/normalize_main.cpp (its own main), built by plain g++ with the sanitizers (their runtimes linked statically)
    and run as a program over the fixture's cases: capacities 0, exact - 1 and exact in heap blocks of exactly that size."""
    exe = str(tmp_path / "normalize_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-omit-frame-pointer", os.path.join(HERE, "normalize_main.cpp"), os.path.join(CSRC, "kgpu_normalize_table.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _, cases = N.fixture_cases()
    lines = []
    for name, raw, exp in cases:
        for form, (want, status) in exp.items():
            lines.append(f"{N.FORMS[form]} {status} {raw.hex() or '-'} {want.hex() or '-'}\n")
    cases_file = tmp_path / "cases.txt"
    cases_file.write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes are linked statically)
    r = subprocess.run([exe, str(cases_file)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"normalize ok: {len(lines)} cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_header_and_constants(tmp_path):
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.kgpu_normalize_unicode_version().decode() == "13.0.0"
    assert (_lib.NORMALIZE_NFC, _lib.NORMALIZE_NFKC, _lib.KGPU_SENT_NOT_NORMALIZED) == (1, 2, 4)
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    assert all(s + "(" in header for s in NEW) and header.index("text normalisation") > header.index("WordPiece ids")
    for d in ("#define KGPU_NORMALIZE_NFC 1", "#define KGPU_NORMALIZE_NFKC 2", "#define KGPU_NORMALIZE_MAX_SEGMENT 64", "#define KGPU_SENT_NOT_NORMALIZED 4"):
        assert d in header, d
    src = tmp_path / "strict.c"
    src.write_text('#include "kanpyo_gpu.h"\nint main(void) { return KGPU_NORMALIZE_NFC + KGPU_NORMALIZE_NFKC == 3 && KGPU_SENT_NOT_NORMALIZED == 4 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, str(src), "-o", str(tmp_path / "strict")], check=True)
    assert subprocess.run([str(tmp_path / "strict")]).returncode == 0


def test_argument_errors_need_no_device():
    L, bad = _lib.lib(), _lib.KGPU_ERR_INVALID_ARG
    a = np.frombuffer(b"abc", dtype=np.uint8)
    off = np.array([0, 3], dtype=np.uint64)
    out, toff, st = np.empty(64, dtype=np.uint8), np.empty(2, dtype=np.uint64), np.empty(1, dtype=np.uint8)
    n, nb = C.c_uint64(0), C.c_uint64(0)
    for form in (0, 3, -1):
        assert L.kgpu_normalize_host(form, a.ctypes.data, 3, out.ctypes.data, 64, C.byref(nb), None) == bad
    assert L.kgpu_normalize_host(1, None, 3, out.ctypes.data, 64, C.byref(nb), None) == bad
    assert L.kgpu_normalize_host(1, a.ctypes.data, 3, None, 64, C.byref(nb), None) == bad
    assert L.kgpu_normalize_host(1, a.ctypes.data, 3, out.ctypes.data, 64, None, None) == bad
    assert L.kgpu_normalize_batch(None, 2, a.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data, C.byref(nb)) == bad
    assert L.kgpu_normalize_text(None, 2, a.ctypes.data, 3, out.ctypes.data, 64, toff.ctypes.data, 2, st.ctypes.data, C.byref(n), C.byref(nb)) == bad
    assert L.kgpu_normalize_device(None, 2, a.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data) == bad
    assert L.kgpu_ctx_sync_normalize(None, C.byref(nb)) == bad
    fake = C.c_void_p(0x1000)   # a handle that must never be looked at: the form and the null pointers are checked first
    assert L.kgpu_normalize_batch(fake, 7, a.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data, C.byref(nb)) == bad
    assert L.kgpu_normalize_batch(fake, 2, a.ctypes.data, None, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data, C.byref(nb)) == bad
    assert L.kgpu_normalize_batch(fake, 2, a.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data, None) == bad
    assert L.kgpu_normalize_text(fake, 0, a.ctypes.data, 3, out.ctypes.data, 64, toff.ctypes.data, 2, st.ctypes.data, C.byref(n), C.byref(nb)) == bad
    assert L.kgpu_normalize_text(fake, 2, None, 3, out.ctypes.data, 64, toff.ctypes.data, 2, st.ctypes.data, C.byref(n), C.byref(nb)) == bad
    assert L.kgpu_normalize_device(fake, 9, a.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data) == bad
    assert L.kgpu_normalize_device(fake, 2, a.ctypes.data, off.ctypes.data, 1, None, 64, toff.ctypes.data, st.ctypes.data) == bad
    assert L.kgpu_normalize_device(fake, 2, out.ctypes.data + 8, off.ctypes.data, 1, out.ctypes.data, 64, toff.ctypes.data, st.ctypes.data) == bad   # d_utf8 inside d_text
    with pytest.raises(ValueError):
        _lib.normalize_form("NFD")
    assert _lib.normalize_form("nfkc") == 2 and _lib.normalize_form("NFC") == 1 and _lib.normalize_form(2) == 2


def test_normalize_host_binding():
    import kanpyo_amd

    assert kanpyo_amd.normalize_host("ﾊﾝｶｸ ＡＢＣ ㈱") == "ハンカク ABC (株)".encode()
    assert kanpyo_amd.normalize_host("ﾊﾝｶｸ ＡＢＣ ㈱", "NFC") == "ﾊﾝｶｸ ＡＢＣ ㈱".encode()
    assert kanpyo_amd.normalize_host(b"e\xcc\x81", "nfc") == "é".encode() and kanpyo_amd.normalize_host(b"\xff\xfe") == b"\xff\xfe" and kanpyo_amd.normalize_host(b"") == b""
    assert kanpyo_amd.normalize_host("ﷺ" * 100) == unicodedata.normalize("NFKC", "ﷺ" * 100).encode() or not N.versions_agree()


# ---- the CLI's options ------------------------------------------------------------------------------------------------------------------------------
def test_cli_options():
    from kanpyo_amd import cli

    for command in ("tokenize", "wakati", "count", "graphviz"):
        assert cli.parse_args([command]).normalize == "none" and cli.parse_args([command, "--normalize", "nfkc"]).normalize == "nfkc"
    assert cli.parse_args(["encode", "--vocab", "v", "--normalize", "nfc", "--split", "device"]).normalize == "nfc"
    a = cli.parse_args(["normalize"])
    assert (a.command, a.form, a.split, a.input) == ("normalize", "nfkc", "host", None) and not hasattr(a, "normalize")
    a = cli.parse_args(["normalize", "ＡＢＣ", "--form", "nfc", "--split", "device", "-c", "x.dict"])
    assert (a.form, a.split, a.input, a.custom_dict) == ("nfc", "device", "ＡＢＣ", "x.dict")
    for argv in (["wakati", "--normalize", "nfd"], ["normalize", "--form", "none"], ["normalize", "--normalize", "nfkc"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)


@pytest.mark.parametrize("command", ["tokenize", "wakati", "count", "encode", "graphviz"])
def test_help_lists_normalize(command, capsys):
    from kanpyo_amd import cli

    with pytest.raises(SystemExit):
        cli.parse_args([command, "--help"])
    assert "--normalize {none,nfc,nfkc}" in capsys.readouterr().out


# ---- the binding over a stub library ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def stub(fixture_dict, monkeypatch):
    from kanpyo_amd import Tokenizer

    lib = StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    tok = Tokenizer(fixture_dict)
    made = [tok]
    yield lib, tok, made
    for obj in reversed(made):
        obj.close()
    gc.collect()


def test_without_normalize_no_normalise_entry_is_reached(stub):
    from kanpyo_amd.tokenizer import pack_sentences

    lib, tok, made = stub
    utf8, offs = pack_sentences(["ab", "cd", "ef"])
    block = b"ab\ncd\nef\n"
    words = tok.words()
    counts = words.counter()
    vocab = words.vocabulary(["<unk>"], unk_id=0)
    made += [words, counts, vocab]
    tok.tokenize_lines_packed(utf8, offs)
    tok.tokenize_lines_packed(utf8, offs, normalize=None)
    tok.tokenize_text_lines(block)
    words.render_packed(utf8, offs)
    words.render_text(block)
    counts.add_packed(utf8, offs)
    counts.add_text(block)
    vocab.encode_packed(utf8, offs)
    vocab.encode_text(block)
    with pytest.raises(UnicodeDecodeError):   # (the stub marks line 2 as not UTF-8)
        tok.tokenize_batch(["ab", "cd", "ef"])
    assert lib.log == ["tokenize_batch_lines", "tokenize_batch_lines", "tokenize_text_lines", "tokenize_batch_words", "tokenize_text_words", "count_batch", "count_text",
                       "encode_batch", "encode_text", "tokenize_batch"]
    assert words.normalize is None and set(lib.seen) == {b"abcdef"}


def test_with_normalize_the_input_is_normalised_first_and_the_status_merged(stub):
    from kanpyo_amd.tokenizer import pack_sentences

    lib, tok, made = stub
    utf8, offs = pack_sentences(["ab", "cd", "ef", "gh"])
    block = b"ab\ncd\nef\ngh\n"
    words = tok.words(normalize="nfkc")
    counts = words.counter()
    vocab = words.vocabulary(["<unk>"], unk_id=0)
    made += [words, counts, vocab]
    assert words.normalize == 2
    merged = [0, 4, 1, 0]   # the tokenizer's 1 stays, the normaliser's 4 shows where the tokenizer said 0
    for call, entry in ((lambda: tok.tokenize_lines_packed(utf8, offs, normalize="NFC"), "tokenize_batch_lines"), (lambda: words.render_packed(utf8, offs), "tokenize_batch_words"),
                        (lambda: vocab.encode_packed(utf8, offs), "encode_batch"), (lambda: tok.words().render_packed(utf8, offs, normalize="NFKC"), "tokenize_batch_words")):
        lib.log.clear()
        lib.seen.clear()
        *_, status = call()
        assert lib.log == [("normalize_batch", 1 if entry == "tokenize_batch_lines" else 2), entry] and lib.seen == [b"ABCDEFGH"] and status.tolist() == merged, entry
    for call, entry in ((lambda: tok.tokenize_text_lines(block, normalize="NFKC"), "tokenize_batch_lines"), (lambda: words.render_text(block), "tokenize_batch_words"),
                        (lambda: vocab.encode_text(block), "encode_batch")):
        lib.log.clear()
        lib.seen.clear()
        *_, status = call()
        assert lib.log == [("normalize_text", 2), entry] and lib.seen == [b"ABCDEFGH"] and status.tolist() == merged, entry
    lib.log.clear()
    assert counts.add_packed(utf8, offs).tolist() == [0, 4, 0, 0] and counts.add_text(block).tolist() == [0, 4, 0, 0]
    assert lib.log == [("normalize_batch", 2), "count_batch", ("normalize_text", 2), "count_batch"]
    lib.log.clear()
    assert tok.normalize(["ab", b"cd"], "NFC") == ["AB", b"CD"] and lib.log == [("normalize_batch", 1)]
    text, toff, status = tok.normalize_packed(utf8, offs)
    assert text.tobytes() == b"ABCDEFGH" and toff.tolist() == [0, 2, 4, 6, 8] and status.tolist() == [0, 4, 0, 0]
    with pytest.raises(ValueError):
        tok.words(normalize="NFD")


def test_cli_warns_about_lines_left_unnormalised(capsys):
    """Every text subcommand names, on stderr, the lines the normaliser left as they were; the numbers run on across the blocks."""
    import io

    from kanpyo_amd import cli

    block = (np.frombuffer(b"a\nb\nc\n", dtype=np.uint8), np.array([0, 2, 4, 6], dtype=np.uint64), np.array([0, 4, 0], dtype=np.uint8))
    out = io.BytesIO()
    assert cli._print_lines(iter([block, block]), out, "panic") == 0 and out.getvalue() == b"a\nb\nc\n" * 2
    assert capsys.readouterr().err == "".join(f"kanpyo_amd: line {k}: a segment is too long to normalise (left unchanged)\n" for k in (2, 5))
    assert cli._each_checked(iter([block[2], (block[0], block[2])]), False) == 0
    assert capsys.readouterr().err.count("left unchanged") == 2
    bad = (block[0], block[1], np.array([1, 4, 0], dtype=np.uint8))   # (nothing behind a line that is not UTF-8 is reported: the run ends there)
    assert cli._print_lines(iter([bad]), io.BytesIO(), "panic") == 101 and capsys.readouterr().err == "panic\n"
