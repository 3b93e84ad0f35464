"""The source alignment without a device (include/kanpyo_gpu.h, "source alignment"): kgpu_normalize_host_aligned -- the definition of every device
result -- against an independent reference built from the generator's segments and unicodedata, and against tests/golden/fixture_align.json;
kgpu_source_spans_host against the header's rules in plain Python on the fixture and on random tokenisations; the capacity protocol of two sizes; the
layout of the two records; the host module alone under AddressSanitizer + UBSan; the binding over a stub library; the CLI's `align`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import normalize_ref as N
from conftest import ROOT, load_golden
from kanpyo_amd import _lib
from normalize_cases import CLEAN, DIRTY, StubLib, same_unicode, view

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "kanpyo_amd", "csrc")
SAME_UNICODE = same_unicode()
NEW = ("kgpu_normalize_host_aligned", "kgpu_normalize_batch_aligned", "kgpu_normalize_text_aligned", "kgpu_normalize_device_aligned", "kgpu_ctx_sync_normalize_aligned",
       "kgpu_source_spans_host", "kgpu_source_spans_device", "kgpu_source_spans_batch")
SEEDS = (11, 20260102, 777)


def _inputs():
    """Every line the reference comparison runs over: the normaliser's fixture (its status 1 and 4 cases included), seeded random strings, the dirty and
    clean pieces of the GPU test alone and joined."""
    _, cases = N.fixture_cases()
    lines = [raw for _, raw, _ in cases]
    for seed in SEEDS:
        lines += [s.encode("utf-8") for s in N.random_strings(seed, 1500)]
    pieces = DIRTY + CLEAN
    lines += [p.encode() for p in pieces] + ["".join(pieces).encode(), "".join(reversed(pieces)).encode(), "".join(p + q for p in DIRTY for q in CLEAN).encode()]
    return lines


# ---- 1. the edits against an independent reference ----------------------------------------------------------------------------------------------------
@SAME_UNICODE
@pytest.mark.parametrize("form", list(N.FORMS))
def test_edits_equal_the_reference(form):
    lines = _inputs()
    with_edits = zero_for_status = 0
    for raw in lines:
        want_out, want_status, want_edits = A.ref_edits(raw, form)
        rc, out, nbytes, status, edits, nedits = A.host_aligned(raw, form)
        assert (rc, out, nbytes, status, edits, nedits) == (0, want_out, len(want_out), want_status, want_edits, len(want_edits)), (raw.hex(), form)
        assert N.host(raw, form)[1] == out   # the unaligned twin gives the same bytes
        with_edits += bool(edits)
        zero_for_status += status != 0
        if status:
            assert not edits and out == raw
    assert with_edits > 1000 and zero_for_status >= 5


def test_edits_describe_the_two_lines():
    """Whatever the Unicode version: the edits are ascending and disjoint, out_len >= 1, and between them the lines are byte-identical."""
    for form in N.FORMS:
        for raw in _inputs():
            rc, out, _, status, edits, _ = A.host_aligned(raw, form)
            assert rc == 0
            op = sp = oc = sc = 0
            for e in edits:
                assert e[0] >= op and e[1] >= sp and e[4] >= 1 and e[5] >= 1 and e[6] >= 1 and e[7] >= 1
                assert out[op : e[0]] == raw[sp : e[1]] and e[0] - op == e[1] - sp
                between = out[op : e[0]].decode("utf-8")
                assert (e[2], e[3]) == (oc + len(between), sc + len(between))
                assert out[e[0] : e[0] + e[4]] != raw[e[1] : e[1] + e[5]]
                assert len(out[e[0] : e[0] + e[4]].decode("utf-8")) == e[6] and len(raw[e[1] : e[1] + e[5]].decode("utf-8")) == e[7]
                op, sp, oc, sc = e[0] + e[4], e[1] + e[5], e[2] + e[6], e[3] + e[7]
            assert out[op:] == raw[sp:]


# ---- 2. the golden file -------------------------------------------------------------------------------------------------------------------------------
def test_fixture_pins_the_granularity():
    g = load_golden("fixture_align.json")
    by = {c["name"]: c for c in g["cases"]}
    for c in g["cases"]:
        raw = bytes.fromhex(c["input"])
        rc, out, _, status, edits, _ = A.host_aligned(raw, c["form"])
        assert (rc, out.hex(), status, [list(e) for e in edits]) == (0, c["output"], c["status"], c["edits"]), c["name"]
    assert [e[4:] for e in by["hankaku_ga"]["edits"]] == [[3, 3, 1, 1], [3, 3, 1, 1], [3, 6, 1, 2], [3, 3, 1, 1]]
    assert by["kabushiki"]["edits"] == [[0, 0, 0, 0, 5, 3, 3, 1]] and by["ufdfa"]["edits"] == [[0, 0, 0, 0, 33, 3, 18, 1]]
    assert by["jamo_l_v_t"]["edits"] == [[0, 0, 0, 0, 3, 9, 1, 3]] and by["e_acute_decomposed"]["edits"] == [[0, 0, 0, 0, 2, 3, 1, 2]]
    assert by["e_acute_precomposed"]["edits"] == [] and by["hangul_precomposed"]["edits"] == [] and by["empty"]["edits"] == [] and by["clean"]["edits"] == []
    # a + dot below + acute is in canonical order already but composes to U+1EA1 U+0301: other bytes, an edit; the swapped order gives the same line
    assert by["reorder_only"]["edits"] == by["reorder_swapped"]["edits"] == [[0, 0, 0, 0, 5, 5, 2, 3]] and by["reorder_only"]["output"] == by["reorder_swapped"]["output"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fixture_align.json")) < 16384


def test_fixture_spans():
    g = load_golden("fixture_align.json")
    names = {c["name"] for c in g["span_cases"]}
    assert {"start_inside_edit_end_at_edit_end", "start_at_edit_end", "end_inside_edit", "end_at_edit_end", "no_edit_before", "eos_after_edit",
            "first_token_not_at_zero", "three_tokens_one_source"} <= names
    for c in g["span_cases"]:
        edits, tokens = A.edit_array(c["edits"]), A.token_array(c["tokens"])
        got = A.host_spans(tokens, [0, len(tokens)], edits, [0, len(edits)])
        assert A.span_lists(got) == c["spans"], c["name"]
        assert A.edit_tuples(edits) == A.host_aligned(bytes.fromhex(c["input"]), c["form"])[4], c["name"]
    by = {c["name"]: c for c in g["span_cases"]}
    assert by["three_tokens_one_source"]["spans"] == [[0, 3, 0, 1]] * 3 + [[3, 0, 1, 4]]   # "(", U+682A, ")" all cover U+3231; the EOS keeps its + 3
    assert by["start_inside_edit_end_at_edit_end"]["spans"] == [[5, 3, 3, 4]] and by["start_at_edit_end"]["spans"] == [[8, 1, 4, 5]]
    assert by["end_inside_edit"]["spans"] == [[4, 4, 2, 4]] and by["end_at_edit_end"]["spans"] == [[0, 4, 0, 2]] and by["no_edit_before"]["spans"] == [[0, 1, 0, 1]]
    assert by["eos_after_edit"]["spans"] == [[9, 0, 5, 8]] and by["first_token_not_at_zero"]["spans"] == [[1, 3, 1, 2], [4, 1, 2, 3]]


@SAME_UNICODE
def test_generator_reproduces_the_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_align_fixture.py"), "--print"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "fixture_align.json"), encoding="ascii") as f:
        assert r.stdout == f.read(), "tests/golden/fixture_align.json is not what tools/gen_align_fixture.py writes"


# ---- 3. the spans against the rules ----------------------------------------------------------------------------------------------------------------------
def test_spans_follow_the_rules_and_are_monotone():
    rng = np.random.default_rng(5)
    strings = [s for seed in SEEDS for s in N.random_strings(seed, 400)] + ["".join(DIRTY + CLEAN), "ﾊﾝｶｸＡＢＣ㈱", "", "東京"]
    records, toff, edits, eoff, want = [], [0], [], [0], []
    for i, s in enumerate(strings):
        rc, out, _, status, ed, _ = A.host_aligned(s.encode("utf-8"), "NFKC" if i % 3 else "NFC")
        assert rc == 0
        recs = A.random_tokens(rng, out.decode("utf-8"), drop_first=i % 5 == 0)
        spans = [A.py_span(t, ed) for t in recs]
        for a, b in zip(spans, spans[1:]):   # starts and ends are each non-decreasing, in bytes and in characters
            assert a[0] <= b[0] and a[2] <= b[2] and a[0] + a[1] <= b[0] + b[1] and a[3] <= b[3], (s, recs, ed)
        src = s.encode("utf-8")
        assert spans[-1][0] == len(src) and spans[-1][2] == len(s) and spans[-1][3] == len(s) + 3   # the EOS: the source line's length
        for t, sp in zip(recs[:-1], spans[:-1]):   # a span is whole source characters, as many as it says
            assert len(src[sp[0] : sp[0] + sp[1]].decode("utf-8")) == sp[3] - sp[2]
        records += recs
        toff.append(len(records))
        edits += ed
        eoff.append(len(edits))
        want += spans
    got = A.host_spans(A.token_array(records), toff, A.edit_array(edits), eoff)
    assert A.span_lists(got) == want and len(want) > 3000 and len(edits) > 1000
    # a batch that does not start at record 0: the spans are those of the records the offsets name
    got = A.host_spans(A.token_array(records), toff[5:], A.edit_array(edits), eoff[5:])
    assert A.span_lists(got) == want[toff[5]:]


# ---- 4. the capacity protocol of two sizes ----------------------------------------------------------------------------------------------------------------
def test_capacity_protocol_of_the_host_function():
    raw = "ｶﾞＡﷺx".encode()
    rc, want, nb, st, edits, ne = A.host_aligned(raw, "NFKC")
    assert (rc, nb, st, ne) == (0, len(want), 0, 3) and len(want) == 3 + 1 + 33 + 1
    cap = _lib.KGPU_ERR_CAPACITY
    assert A.host_aligned(raw, "NFKC", nb - 1, ne) == (cap, b"", nb, 0, [], ne)       # the text too small
    assert A.host_aligned(raw, "NFKC", nb, ne - 1) == (cap, b"", nb, 0, [], ne)       # the edits too small
    assert A.host_aligned(raw, "NFKC", nb - 1, ne - 1) == (cap, b"", nb, 0, [], ne)   # both
    assert A.host_aligned(raw, "NFKC", 0, 0) == (cap, b"", nb, 0, [], ne)
    assert A.host_aligned(raw, "NFKC", nb, ne) == (0, want, nb, 0, edits, ne)
    assert A.host_aligned(b"", "NFC", 0, 0) == (0, b"", 0, 0, [], 0)
    assert A.host_aligned(b"abc", "NFC", 3, 0) == (0, b"abc", 3, 0, [], 0)             # clean text needs no edit room
    assert A.host_aligned(b"\xff", "NFC", 0, 0) == (cap, b"", 1, 1, [], 0)            # an invalid line is copied: its own length, no edits
    assert A.host_aligned(b"\xff", "NFC", 1, 0) == (0, b"\xff", 1, 1, [], 0)
    long_line = ("a" + "\u0301" * 65 + "Ａ").encode()
    assert A.host_aligned(long_line, "NFKC", len(long_line), 0) == (0, long_line, len(long_line), 4, [], 0)


def test_argument_errors_need_no_device():
    L, bad = _lib.lib(), _lib.KGPU_ERR_INVALID_ARG
    a = np.frombuffer(b"abc", dtype=np.uint8)
    off = np.array([0, 3], dtype=np.uint64)
    out, toff, st, ed, eoff = np.empty(64, dtype=np.uint8), np.empty(2, dtype=np.uint64), np.empty(1, dtype=np.uint8), np.empty(4, dtype=A.EDIT_DTYPE), np.empty(2, dtype=np.uint64)
    n, nb, ne = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    P = lambda x: x.ctypes.data   # noqa: E731
    assert L.kgpu_normalize_host_aligned(3, P(a), 3, P(out), 64, C.byref(nb), None, P(ed), 4, C.byref(ne)) == bad
    assert L.kgpu_normalize_host_aligned(1, P(a), 3, P(out), 64, C.byref(nb), None, None, 4, C.byref(ne)) == bad
    assert L.kgpu_normalize_host_aligned(1, P(a), 3, P(out), 64, C.byref(nb), None, P(ed), 4, None) == bad
    fake = C.c_void_p(0x1000)   # a handle that must never be looked at
    assert L.kgpu_normalize_batch_aligned(None, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), C.byref(nb), P(ed), 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_batch_aligned(fake, 7, P(a), P(off), 1, P(out), 64, P(toff), P(st), C.byref(nb), P(ed), 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_batch_aligned(fake, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), C.byref(nb), None, 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_batch_aligned(fake, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), C.byref(nb), P(ed), 4, None, C.byref(ne)) == bad
    assert L.kgpu_normalize_batch_aligned(fake, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), C.byref(nb), P(ed), 4, P(eoff), None) == bad
    assert L.kgpu_normalize_text_aligned(None, 2, P(a), 3, P(out), 64, P(toff), 2, P(st), C.byref(n), C.byref(nb), P(ed), 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_text_aligned(fake, 0, P(a), 3, P(out), 64, P(toff), 2, P(st), C.byref(n), C.byref(nb), P(ed), 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_text_aligned(fake, 2, P(a), 3, P(out), 64, P(toff), 2, P(st), C.byref(n), C.byref(nb), None, 4, P(eoff), C.byref(ne)) == bad
    assert L.kgpu_normalize_device_aligned(None, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), P(ed), 4, P(eoff)) == bad
    assert L.kgpu_normalize_device_aligned(fake, 9, P(a), P(off), 1, P(out), 64, P(toff), P(st), P(ed), 4, P(eoff)) == bad
    assert L.kgpu_normalize_device_aligned(fake, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), None, 4, P(eoff)) == bad
    assert L.kgpu_normalize_device_aligned(fake, 2, P(a), P(off), 1, P(out), 64, P(toff), P(st), P(ed), 4, None) == bad
    assert L.kgpu_ctx_sync_normalize_aligned(None, C.byref(nb), C.byref(ne)) == bad
    assert L.kgpu_source_spans_device(None, P(out), P(toff), 1, P(ed), P(eoff), P(out), 4) == bad
    assert L.kgpu_source_spans_device(fake, P(out), None, 1, P(ed), P(eoff), P(out), 4) == bad
    assert L.kgpu_source_spans_device(fake, P(out), P(toff), 1, P(ed), None, P(out), 4) == bad
    assert L.kgpu_source_spans_batch(None, P(out), P(toff), 1, P(ed), P(eoff), P(out)) == bad
    assert L.kgpu_source_spans_batch(fake, P(out), None, 1, P(ed), P(eoff), P(out)) == bad
    backwards = np.array([3, 1], dtype=np.uint64)
    assert L.kgpu_source_spans_batch(fake, P(out), P(backwards), 1, P(ed), P(off), P(out)) == bad


# ---- 5. ABI ----------------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_header_and_layout(tmp_path):
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes is not None, s
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    assert all(s + "(" in header for s in NEW) and header.index("source alignment") > header.index("text normalisation")
    assert C.sizeof(_lib.NormEdit) == A.EDIT_DTYPE.itemsize == 24 and C.sizeof(_lib.Span) == A.SPAN_DTYPE.itemsize == 16
    assert [(n, A.EDIT_DTYPE.fields[n][1]) for n in A.EDIT_FIELDS] == [(n, getattr(_lib.NormEdit, n).offset) for n, _ in _lib.NormEdit._fields_]
    assert [(n, A.SPAN_DTYPE.fields[n][1]) for n in A.SPAN_FIELDS] == [(n, getattr(_lib.Span, n).offset) for n, _ in _lib.Span._fields_]
    exe = str(tmp_path / "align_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "align_layout.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "align layout ok" in r.stdout, r.stdout
    with open(os.path.join(CSRC, "Makefile"), encoding="utf-8") as f:
        assert f.read().count("kgpu_align.hip") == 2   # SRCS and the resource-usage target


def _edit_words(edits):
    return f"{len(edits)}" + "".join(" " + " ".join(map(str, e)) for e in edits)


def test_host_module_alone_under_asan_ubsan(tmp_path):
    """kgpu_normalize_table.cpp and tests/c_abi/align_main.cpp (its own main), built by plain g++ with the sanitizers (their runtimes linked statically)
    and run as a program over both fixtures and the random strings: every buffer a heap block of exactly the size the call is told."""
    exe = str(tmp_path / "align_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-omit-frame-pointer", os.path.join(HERE, "align_main.cpp"), os.path.join(CSRC, "kgpu_normalize_table.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    g = load_golden("fixture_align.json")
    lines = []
    for c in g["cases"]:
        lines.append(f"N {N.FORMS[c['form']]} {c['status']} {c['input'] or '-'} {c['output'] or '-'} {_edit_words(c['edits'])}\n")
    for c in g["span_cases"]:
        lines.append(f"S {_edit_words(c['edits'])} {len(c['tokens'])}" + "".join(" " + " ".join(map(str, t)) for t in c["tokens"])
                     + "".join(" " + " ".join(map(str, s)) for s in c["spans"]) + "\n")
    agree = N.versions_agree()
    for form in N.FORMS:
        for raw in _inputs()[:1200]:   # the normaliser's fixture and the first seed's strings
            out, status, edits = A.ref_edits(raw, form) if agree else (lambda h: (h[1], h[3], h[4]))(A.host_aligned(raw, form))
            lines.append(f"N {N.FORMS[form]} {status} {raw.hex() or '-'} {out.hex() or '-'} {_edit_words(edits)}\n")
    cases_file = tmp_path / "cases.txt"
    cases_file.write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes are linked statically)
    r = subprocess.run([exe, str(cases_file)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"align ok: {len(lines)} cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 6. the binding over a stub library, and the CLI ---------------------------------------------------------------------------------------------------------
class AlignStub(StubLib):
    """StubLib with the aligned entries: the normalise entry's text, no edits; spans of zeros."""

    def kgpu_normalize_batch_aligned(self, h, form, u, o, n, text, cap, toff, st, got, edits, ecap, eoff, ne):
        rc = self.kgpu_normalize_batch(h, form, u, o, n, text, cap, toff, st, got)
        self.log[-1] = ("normalize_batch_aligned", form)
        ne._obj.value = 0
        if rc == 0:
            view(eoff, np.uint64, n + 1)[:] = 0
        return rc

    def kgpu_source_spans_batch(self, h, tokens, toff, n, edits, eoff, spans):
        self.log.append("source_spans_batch")
        t = view(toff, np.uint64, n + 1)
        view(spans, np.uint8, int(t[n] - t[0]) * 16)[:] = 0
        return 0


@pytest.fixture
def stub(fixture_dict, monkeypatch):
    import gc

    from kanpyo_amd import Tokenizer

    lib = AlignStub()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    tok = Tokenizer(fixture_dict)
    yield lib, tok
    tok.close()
    gc.collect()


def test_tokenize_aligned_is_normalise_tokenize_spans(stub):
    import kanpyo_amd

    lib, tok = stub
    rows = tok.tokenize_aligned(["ab", "cd"], normalize="nfc")
    assert lib.log == [("normalize_batch_aligned", 1), "tokenize_batch", "source_spans_batch"] and lib.seen == [b"ABCD"]
    assert [len(r) for r in rows] == [1, 1] and isinstance(rows[0][0], kanpyo_amd.AlignedToken)
    a = rows[0][0]
    assert a.token == kanpyo_amd.Token(0, kanpyo_amd.TokenClass.Dummy, 0, 0, 0, "EOS") and a.source_surface == "EOS"
    assert (a.source_position, a.source_byte_len, a.source_start, a.source_end) == (0, 0, 0, 0)
    with pytest.raises(Exception):   # a frozen dataclass
        a.source_start = 1
    lib.log.clear()
    tok.tokenize_batch(["ab", "cd"])
    tok.tokenize_batch(["ab", "cd"], normalize="NFKC")
    assert lib.log == ["tokenize_batch", ("normalize_batch", 2), "tokenize_batch"]   # tokenize_batch reaches none of the new entries
    with pytest.raises(ValueError):
        tok.tokenize_aligned(["ab"], normalize="NFD")


def test_normalize_host_aligned_binding():
    import kanpyo_amd

    out, edits = kanpyo_amd.normalize_host_aligned("xＡy㈱z")
    assert out == "xAy(株)z".encode() and edits.dtype == A.EDIT_DTYPE and A.edit_tuples(edits) == [(1, 1, 1, 1, 1, 3, 1, 1), (3, 5, 3, 3, 5, 3, 3, 1)]
    out, edits = kanpyo_amd.normalize_host_aligned("xＡy㈱z", "NFC")
    assert out == "xＡy㈱z".encode() and len(edits) == 0
    assert kanpyo_amd.normalize_host_aligned(b"\xff\xfe")[0] == b"\xff\xfe" and kanpyo_amd.normalize_host_aligned(b"")[0] == b""


def test_cli_lists_align(capsys):
    from kanpyo_amd import cli

    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    assert "align" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.parse_args(["align", "--help"])
    out = capsys.readouterr().out
    assert "--form {nfkc,nfc}" in out and "--normalize" not in out
    a = cli.parse_args(["align", "ＡＢＣ", "--form", "nfc", "-c", "x.dict"])
    assert (a.command, a.form, a.input, a.custom_dict) == ("align", "nfc", "ＡＢＣ", "x.dict")
    assert cli.parse_args(["align"]).form == "nfkc"
    with pytest.raises(SystemExit):
        cli.parse_args(["align", "--normalize", "nfkc"])
