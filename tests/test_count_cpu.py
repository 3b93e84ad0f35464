"""The host side of the word counts (include/kanpyo_gpu.h, "word counts") without a device: tests/count_ref.py against the hand-derived
tests/golden/fixture_counts.json and against a Counter over the wakati reference's lines; the merge and the order of the read-out through the
kgpu_debug_counts_order hook; the new symbols; the C layout of the new structs; the CLI's argument parsing."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import count_ref as CR
import words_ref as W
from conftest import ROOT, fixture_dict_parts, load_golden
from golden_cases import TOKEN_DTYPE, fixture_tables, golden_records
from kanpyo_amd import _lib

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
NEW = ("kgpu_counts_create", "kgpu_counts_destroy", "kgpu_counts_reset", "kgpu_counts_get_info", "kgpu_count_batch", "kgpu_count_text",
       "kgpu_count_words_device", "kgpu_ctx_sync_count", "kgpu_counts_read")


def test_reference_reproduces_the_golden_counts():
    p, known, unk = fixture_tables()
    cases = load_golden("fixture_counts.json")["cases"]
    assert len(cases) >= 7 and any(n > 1 for c in cases for _, n in c["counts"]), "the golden needs a repeated word"
    for c in cases:
        spec = W.Spec(c["field"], c["filter"], c["names"])
        got = CR.count(*golden_records(c["sentences"]), known, unk, len(p["morphs"]), len(p["unk_morphs"]), spec, p["sorted_keywords"], own_records=True)
        assert CR.ordered(got) == [(w.encode(), n) for w, n in c["counts"]], c
        assert CR.ordered(got, 2) == [(w.encode(), n) for w, n in c["counts"]][:2]


def test_reference_equals_a_counter_over_the_wakati_lines():
    """Where no word is empty or holds the separator, counting the words of words_ref.render's lines is the same thing."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    nk, nu = len(known.morph_features), len(unk.morph_features)
    keys = synth.record_surfaces(sd)
    utf8, offs = pack_sentences(synth.make_corpus(sd, 300, 3, "cfg2") + synth.make_corpus(sd, 20, 4, "cfg3"))
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 1)
    for field, filt, names in ((W.SURFACE, W.ALL, ()), (7, W.DROP, ("助詞", "助動詞", "記号")), (0, W.ALL, ()), (8, W.KEEP, ("名詞",))):
        spec = W.Spec(field, filt, names, sep=b"\x01")
        got = CR.count(utf8, offs, exp.tokens, exp.offsets, known, unk, nk, nu, spec, keys, own_records=True)
        text, _ = W.render(utf8, offs, exp.tokens, exp.offsets, known, unk, nk, nu, spec)
        words = [w for line in text.split(b"\n") for w in line.split(b"\x01") if line]
        assert b"" not in got and not any(b"\x01" in w or b"\n" in w for w in got)
        assert got == Counter(words) and sum(got.values()) > 1000, (field, filt)


def test_reference_counts_a_known_record_under_its_key():
    """Rule 2's sharpening on crafted records: a known record with an id is counted under the dictionary's key whatever its position and
    length say; an unknown record and a record without a row under their bytes; the empty word is a key."""
    p, known, unk = fixture_tables()
    raw = b"ab cd"
    recs = [(1, 1, 0, 2), (1, 1, 3, 1), (2, 1, 0, 0), (0, 1, 0, 2), (1, 2, 3, 2), (0, 2, 5, 0), (0, 0, 99, 99), (0, 1, 2, 0)]
    tokens = np.zeros(len(recs), dtype=TOKEN_DTYPE)
    for i, (tid, cls, pos, bl) in enumerate(recs):
        tokens[i] = (tid, cls, pos, 0, 0, bl)
    got = CR.count(raw, [0, 5], tokens, [0, len(recs)], known, unk, 3, 2, W.Spec(), p["sorted_keywords"])
    assert got == Counter({"テスト".encode(): 2, "辞書".encode(): 1, b"ab": 1, b"cd": 1, b"": 2})
    with pytest.raises(AssertionError):
        CR.count(raw, [0, 5], tokens, [0, len(recs)], known, unk, 3, 2, W.Spec(), p["sorted_keywords"], own_records=True)
    with pytest.raises(ValueError):
        CR.count(raw, [0, 5], tokens[:1], [0, 1], known, unk, 0, 2, W.Spec(), p["sorted_keywords"])


# ---- the merge and the order of the read-out ---------------------------------------------------------------------------------------------
def counts_order(entries, top=0):
    """kgpu_debug_counts_order over [(bytes, count)] -> [(bytes, count)], through the exact-sizes protocol."""
    L = _lib.lib()
    blob = np.frombuffer(b"".join(w for w, _ in entries) + b"\xee", dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(w) for w, _ in entries])]).astype(np.uint64)
    cnts = np.array([n for _, n in entries] + [0], dtype=np.uint64)
    ne, nb = C.c_uint64(0), C.c_uint64(0)
    args = (blob.ctypes.data, offs.ctypes.data, cnts.ctypes.data, len(entries), top)
    rc = L.kgpu_debug_counts_order(*args, None, 0, None, None, 0, C.byref(ne), C.byref(nb))
    if rc == _lib.KGPU_OK:
        assert ne.value == 0 and nb.value == 0
        return []
    assert rc == _lib.KGPU_ERR_CAPACITY
    n, b = int(ne.value), int(nb.value)
    words = np.full(b + 8, 0xAB, dtype=np.uint8)
    woff = np.zeros(n + 1, dtype=np.uint64)
    out = np.zeros(n + 1, dtype=np.uint64)
    if n > 1:   # short by one entry, and short by one byte: nothing written, the same sizes
        assert L.kgpu_debug_counts_order(*args, words.ctypes.data, b, woff.ctypes.data, out.ctypes.data, n - 1, C.byref(ne), C.byref(nb)) == _lib.KGPU_ERR_CAPACITY
        assert (ne.value, nb.value) == (n, b) and (words == 0xAB).all()
    if b:
        assert L.kgpu_debug_counts_order(*args, words.ctypes.data, b - 1, woff.ctypes.data, out.ctypes.data, n, C.byref(ne), C.byref(nb)) == _lib.KGPU_ERR_CAPACITY
        assert (ne.value, nb.value) == (n, b) and (words == 0xAB).all()
    assert L.kgpu_debug_counts_order(*args, words.ctypes.data, b, woff.ctypes.data, out.ctypes.data, n, C.byref(ne), C.byref(nb)) == _lib.KGPU_OK
    assert (ne.value, nb.value) == (n, b) and (words[b:] == 0xAB).all() and int(woff[n]) == b
    raw = words.tobytes()
    return [(raw[int(woff[i]) : int(woff[i + 1])], int(out[i])) for i in range(n)]


def test_order_hook_merges_and_orders():
    # equal bytes arriving as several entries are merged
    assert counts_order([(b"x", 2), (b"y", 1), (b"x", 3), (b"y", 1), (b"x", 1)]) == [(b"x", 6), (b"y", 2)]
    # ties are ordered by bytes; a prefix comes before its extension; bytes are unsigned
    assert counts_order([(b"b", 1), (b"ab", 1), (b"a", 1), (b"\xff", 1), (b"abc", 1), (b"\x7f", 1)]) == \
        [(b"a", 1), (b"ab", 1), (b"abc", 1), (b"b", 1), (b"\x7f", 1), (b"\xff", 1)]
    # the count decides first
    assert counts_order([(b"a", 1), (b"z", 5), (b"m", 3)]) == [(b"z", 5), (b"m", 3), (b"a", 1)]
    # the empty word is a key, and the smallest
    assert counts_order([(b"a", 2), (b"", 2), (b"", 1), (b"\0", 3)]) == [(b"", 3), (b"\0", 3), (b"a", 2)]
    # "a" against "a\0": two entries
    assert counts_order([(b"a\0", 4), (b"a", 4), (b"a", 1)]) == [(b"a", 5), (b"a\0", 4)]
    # 64-bit counts
    assert counts_order([(b"q", 2**40), (b"q", 2**40), (b"r", 2**41 + 1)]) == [(b"r", 2**41 + 1), (b"q", 2**41)]
    assert counts_order([]) == []


def test_order_hook_top_cuts_after_the_sort():
    entries = [(b"d", 2), (b"c", 2), (b"b", 2), (b"a", 2), (b"e", 9), (b"c", 0)]
    full = counts_order(entries)
    assert full == [(b"e", 9), (b"a", 2), (b"b", 2), (b"c", 2), (b"d", 2)]
    assert counts_order(entries, 3) == full[:3]        # inside the tie: its smallest bytes survive
    assert counts_order(entries, 1) == full[:1] and counts_order(entries, 5) == full and counts_order(entries, 99) == full
    rng = np.random.default_rng(1)
    words = [bytes(rng.integers(0, 4, size=int(rng.integers(0, 4)), dtype=np.uint8)) for _ in range(400)]
    entries = [(w, int(rng.integers(1, 4))) for w in words]
    want = Counter()
    for w, n in entries:
        want[w] += n
    assert counts_order(entries) == CR.ordered(want) and counts_order(entries[::-1], 7) == CR.ordered(want, 7)


def key_table(index_blob, n_morphs):
    """kgpu_debug_key_table -> the dictionary's key of every id 1..n_morphs (bytes)."""
    L = _lib.lib()
    blob = np.frombuffer(index_blob, dtype=np.uint8)
    off = np.zeros(n_morphs + 1, dtype=np.uint64)
    got = C.c_uint64(0)
    rc = L.kgpu_debug_key_table(blob.ctypes.data, blob.size, n_morphs, None, 0, C.byref(got), off.ctypes.data)
    assert rc in (_lib.KGPU_OK, _lib.KGPU_ERR_CAPACITY)
    keys = np.zeros(max(int(got.value), 1), dtype=np.uint8)
    assert L.kgpu_debug_key_table(blob.ctypes.data, blob.size, n_morphs, keys.ctypes.data, keys.size, C.byref(got), off.ctypes.data) == _lib.KGPU_OK
    raw, o = keys.tobytes(), off.tolist()
    return [raw[o[i] : o[i + 1]] for i in range(n_morphs)]


def test_key_table_names_every_id_by_its_surface(fixture_dict):
    """The read-out's id -> key table: the fixture's keywords, and on a synthetic dictionary every record's surface, duplicates included."""
    from kanpyo_amd import synth

    p = fixture_dict_parts()
    assert key_table(fixture_dict.index_dict, len(p["morphs"])) == [k.encode() for k in p["sorted_keywords"]]
    sd = synth.build_dict(20000, seed=5)
    want = [s.encode() for s in synth.record_surfaces(sd)]
    assert len(set(want)) < len(want), "the dictionary needs surfaces with several records"
    assert key_table(sd.dict.index_dict, len(want)) == want
    assert key_table(sd.dict.index_dict, len(want) - 5) == want[:-5]   # (fewer morphs than ids: the ids beyond are left out)


def test_read_out_argument_errors():
    L = _lib.lib()
    bad = _lib.KGPU_ERR_INVALID_ARG
    ne, nb = C.c_uint64(0), C.c_uint64(0)
    assert L.kgpu_debug_counts_order(None, None, None, 1, 0, None, 0, None, None, 0, C.byref(ne), C.byref(nb)) == bad
    assert L.kgpu_debug_counts_order(None, None, None, 0, 0, None, 0, None, None, 0, None, C.byref(nb)) == bad
    out = C.c_void_p()
    assert L.kgpu_counts_create(None, None, C.byref(out)) == bad and L.kgpu_counts_reset(None) == bad
    assert L.kgpu_counts_get_info(None, None) == bad and L.kgpu_count_batch(None, None, None, 0, None) == bad
    assert L.kgpu_count_text(None, None, 0, None, 0, C.byref(ne)) == bad and L.kgpu_ctx_sync_count(None, None) == bad
    assert L.kgpu_count_words_device(None, None, None, None, 0, None, None) == bad
    assert L.kgpu_counts_read(None, 0, None, 0, None, None, 0, C.byref(ne), C.byref(nb)) == bad
    L.kgpu_counts_destroy(None)


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes, s
    assert hasattr(L, "kgpu_debug_counts_order") and "kgpu_debug_counts_order" not in _lib.SYMBOLS
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    assert "kgpu_debug_counts_order" not in header and all(s + "(" in header for s in NEW)


def test_counts_structs_layout_matches_the_ctypes_mirrors(tmp_path):
    exe = str(tmp_path / "counts_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "counts_layout.c"), "-o", exe], check=True)
    fields, consts = {"kgpu_counts_opts": {}, "kgpu_counts_info": {}}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, a, b = line.split()
        if st == "const":
            consts[f] = int(a)
        else:
            fields[st][f] = (int(a), int(b))
    for name, mirror in (("kgpu_counts_opts", _lib.CountsOpts), ("kgpu_counts_info", _lib.CountsInfo)):
        got = fields[name]
        assert got.pop("-") == (0, C.sizeof(mirror))
        assert set(got) == {n for n, _ in mirror._fields_}
        for f, (off, size) in got.items():
            m = getattr(mirror, f)
            assert (m.offset, m.size) == (off, size), (name, f)
    assert consts == {"KGPU_COUNTS_DEFAULT_SLOTS": _lib.KGPU_COUNTS_DEFAULT_SLOTS, "KGPU_COUNTS_DEFAULT_KEY_BYTES": _lib.KGPU_COUNTS_DEFAULT_KEY_BYTES}
    assert consts["KGPU_COUNTS_DEFAULT_SLOTS"] == 1 << 22 and consts["KGPU_COUNTS_DEFAULT_KEY_BYTES"] == 256 << 20


def test_counts_consumer_is_strict_c99_and_links(tmp_path):
    exe = str(tmp_path / "counts_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "counts_consumer.c"), "-o", exe,
                    "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    syms = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    used = {w for line in syms.splitlines() for w in line.split() if w.startswith("kgpu_")}
    assert {"kgpu_counts_create", "kgpu_counts_destroy", "kgpu_counts_reset", "kgpu_counts_get_info", "kgpu_count_batch", "kgpu_count_text", "kgpu_counts_read"} <= used


def test_cli_argument_parsing():
    from kanpyo_amd import cli

    a = cli.parse_args(["count"])
    assert (a.command, a.input, a.field, a.drop, a.keep, a.top, a.split, a.skip_invalid) == ("count", None, None, [], [], None, "host", False)
    a = cli.parse_args(["count", "すもも", "-c", "x.dict", "--reading", "--drop", "助詞,助動詞,記号", "--top", "20", "--split", "device", "--skip-invalid"])
    assert (a.input, a.custom_dict, a.field, a.drop, a.keep, a.top, a.split, a.skip_invalid) == ("すもも", "x.dict", 7, ["助詞", "助動詞", "記号"], [], 20, "device", True)
    assert cli.parse_args(["count", "--base-form"]).field == 6 and cli.parse_args(["count", "--pronunciation"]).field == 8
    assert cli.parse_args(["count", "--field", "0", "--keep", "名詞"]).keep == ["名詞"]
    for argv in (["count", "--field", "3", "--reading"], ["count", "--drop", "a", "--keep", "b"], ["count", "--field", "-1"], ["count", "--top", "0"],
                 ["count", "--top", "x"], ["count", "--top", "-3"], ["count", "--split", "gpu"], ["count", "--separator", "|"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    # the other subcommands are what they were
    assert cli.parse_args([]).command == "tokenize" and cli.parse_args(["wakati", "--reading"]).field == 7 and not hasattr(cli.parse_args(["wakati"]), "top")
