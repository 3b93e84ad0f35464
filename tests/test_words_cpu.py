"""The host side of the wakati output (include/kanpyo_gpu.h, "wakati-gaki") without a device: tests/words_ref.py against the hand-derived
golden lines; the per-row word table of kgpu_words_create (through the kgpu_debug_word_table hook) against words_ref's word choice and drop
decision, row by row; every argument error of kgpu_words_create; the CLI's argument parsing; the C consumer and the struct layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import words_ref as W
from conftest import ROOT, load_golden
from golden_cases import TOKEN_DTYPE, fixture_tables
from kanpyo_amd import _lib
from kanpyo_amd.dictfile import MorphFeatureTable

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
SURFACE_BIT, DROPPED_BIT = 1 << 30, 1 << 31

def golden_spec(c):
    return W.Spec(c["field"], c["filter"], c["names"], c["separator"])


def test_reference_reproduces_the_golden_lines():
    p, known, unk = fixture_tables()
    tokens_of = {c["input"]: c["tokens"] for c in load_golden("fixture_tokens.json")["cases"]}
    cases = load_golden("fixture_words.json")["cases"]
    assert len(cases) >= 8
    for c in cases:
        recs = tokens_of[c["input"]]
        tokens = np.zeros(len(recs), dtype=TOKEN_DTYPE)
        for i, (tid, cls, pos, start, end, surface) in enumerate(recs):
            tokens[i] = (tid, cls, pos, start, end, 0 if cls == 0 else len(surface.encode()))
        raw = c["input"].encode()
        text, toff = W.render(raw, [0, len(raw)], tokens, [0, len(recs)], known, unk, len(p["morphs"]), len(p["unk_morphs"]), golden_spec(c))
        assert text == c["line"].encode(), c
        assert toff.tolist() == [0, len(text)]


def test_reference_rules_on_crafted_records():
    """EOS records with any id, position and length; zero-length surfaces; a surface that is a space; rejected records."""
    _, known, unk = fixture_tables()
    raw = b"ab cd"
    recs = [(0, 0, 999, 77), (1, 1, 0, 2), (5, 0, 0, 0), (0, 1, 2, 1), (1, 1, 3, 0), (-7, 0, 1, 1), (1, 2, 3, 2)]
    tokens = np.zeros(len(recs), dtype=TOKEN_DTYPE)
    for i, (tid, cls, pos, bl) in enumerate(recs):
        tokens[i] = (tid, cls, pos, 0, 0, bl)
    args = (raw, [0, 5], tokens, [0, len(recs)], known, unk, 3, 8)
    assert W.render(*args, W.Spec())[0] == b"ab    cd\n"                     # "ab", " ", "", "cd": the empty word makes two separators meet
    assert W.render(*args, W.Spec(1, sep="/"))[0] == b"k1/ /k1/u1\n"        # id 0 has no row: the surface
    assert W.render(*args, W.Spec(filter=W.KEEP, names=["名詞"]))[0] == b"ab \n"   # id 0 matches no name: KEEP drops it
    assert W.render(*args, W.Spec(filter=W.DROP, names=["名詞"]))[0] == b"  cd\n"  # ... and DROP keeps it
    for bad in [(4, 1, 0, 1), (-1, 1, 0, 1), (9, 2, 0, 1), (1, 3, 0, 1), (1, 1, 6, 0), (1, 1, 4, 2)]:
        t = np.zeros(1, dtype=TOKEN_DTYPE)
        t[0] = (bad[0], bad[1], bad[2], 0, 0, bad[3])
        with pytest.raises(ValueError):
            W.render(raw, [0, 5], t, [0, 1], known, unk, 3, 8, W.Spec())
    with pytest.raises(ValueError):
        W.render(raw, [0, 5], tokens, [2, 1], known, unk, 3, 8, W.Spec())


# ---- the word table ---------------------------------------------------------------------------------------------------------------------
def make_spec(field=-1, filt=0, names=(), separator=0, size=None):
    """-> (_lib.WordsSpec, keep-alive arrays) with everything as given (no checks: the library's are under test)."""
    enc = [n.encode() if isinstance(n, str) else n for n in names]
    blob = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.uint64)
    spec = _lib.WordsSpec(C.sizeof(_lib.WordsSpec) if size is None else size, field, filt, separator, blob.ctypes.data, offs.ctypes.data, len(enc))
    return spec, (blob, offs)


def word_table(known, unk, n_known, n_unk, spec):
    """kgpu_debug_word_table -> (rc, entries[rows, 2] uint32, pool bytes, separator)."""
    L = _lib.lib()
    a, b = np.frombuffer(known.encode(), dtype=np.uint8), np.frombuffer(unk.encode(), dtype=np.uint8)
    entries = np.zeros((n_known + n_unk, 2), dtype=np.uint32)
    got, sep = C.c_uint64(0), C.c_uint32(0)
    args = (a.ctypes.data, a.size, b.ctypes.data, b.size, n_known, n_unk, C.byref(spec), entries.ctypes.data)
    rc = L.kgpu_debug_word_table(*args, None, 0, C.byref(got), C.byref(sep))
    if rc == _lib.KGPU_ERR_CAPACITY:
        pool = np.zeros(got.value, dtype=np.uint8)
        rc = L.kgpu_debug_word_table(*args, pool.ctypes.data, pool.size, C.byref(got), C.byref(sep))
        return rc, entries, pool.tobytes(), sep.value
    return rc, entries, b"", sep.value


def check_table(known, unk, n_known, n_unk, field, filt, names):
    spec, keep = make_spec(field, filt, names)
    rc, entries, pool, sep = word_table(known, unk, n_known, n_unk, spec)
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    assert sep == 32
    ref = W.Spec(field, filt, names)
    rows = [known.features(i) for i in range(1, n_known + 1)] + [unk.features(i) for i in range(1, n_unk + 1)]
    used = set()
    for r, feats in enumerate(rows):
        off, lf = int(entries[r, 0]), int(entries[r, 1])
        want = W.row_word(feats, ref)
        assert bool(lf & DROPPED_BIT) == W.row_dropped(feats, ref), (r, feats)
        if want is None:
            assert lf & SURFACE_BIT, (r, feats)
        else:
            n = lf & (SURFACE_BIT - 1)
            assert not lf & SURFACE_BIT and pool[off : off + n] == want, (r, feats, pool[off : off + n])
            used.add(want)
    assert len(pool) == sum(len(w) for w in used), "the pool holds more than the distinct names once each"
    return entries


SPECS = [(-1, W.ALL, ()), (0, W.ALL, ()), (6, W.ALL, ()), (7, W.DROP, ("助詞", "助動詞", "記号")), (8, W.KEEP, ("感動詞",)), (40, W.KEEP, ()),
         (1, W.DROP, ()), (3, W.KEEP, ("名詞", "動詞", "no such name"))]


def test_word_table_on_a_synthetic_dictionary():
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    nk, nu = len(known.morph_features), len(unk.morph_features)
    assert nk >= 20000
    dropped_some = False
    for field, filt, names in SPECS:
        e = check_table(known, unk, nk, nu, field, filt, names)
        d = (e[:, 1] & DROPPED_BIT) != 0
        dropped_some |= bool(d.any() and not d.all())
    assert dropped_some
    check_table(known, unk, nk - 3, 1, 7, W.DROP, ("名詞",))   # fewer morphs than rows


def test_word_table_on_a_crafted_table():
    big = "長" * 3400   # 10 200 bytes
    known = MorphFeatureTable.from_features([
        [], ["名詞"], ["名詞", "*"], ["名詞", ""], ["名", "x", "y"], ["名詞一般", big, "*", ""], ["*"], [""], ["", "*", big],
        ["助詞", "x", "y", "z", "*", "*", "base", "ヨミ", "ヨミ"], [big], ["名詞"] * 41,
    ])
    unk = MorphFeatureTable.from_features([["未知語", "u"], [], ["名詞", big, "x", "*", "*", "*", "*"]])
    nk, nu = len(known.morph_features), len(unk.morph_features)
    for field in (-1, 0, 1, 2, 3, 6, 7, 40, 41, 2**31 - 1):
        for filt, names in ((W.ALL, ("名詞",)), (W.DROP, ("名詞",)), (W.KEEP, ("名詞",)), (W.DROP, ("名詞一般", "")), (W.KEEP, ("名", "*")), (W.DROP, ()), (W.KEEP, ()),
                            (W.KEEP, (big,))):
            check_table(known, unk, nk, nu, field, filt, names)
    # "名" is a prefix of the listed "名詞" and "名詞一般" has it as a prefix: neither matches
    e = check_table(known, unk, nk, nu, -1, W.DROP, ("名詞",))
    assert [bool(x & DROPPED_BIT) for x in e[:6, 1]] == [False, True, True, True, False, False]
    # the tables' own validation still holds: a row naming a missing name, fewer rows than morphs
    spec, keep = make_spec()
    assert word_table(MorphFeatureTable([[5]], ["", "a"]), unk, 1, nu, spec)[0] == _lib.KGPU_ERR_BAD_DICT
    assert word_table(known, unk, nk + 1, nu, spec)[0] == _lib.KGPU_ERR_BAD_DICT


def test_create_argument_errors():
    L = _lib.lib()
    p, known, unk = fixture_tables()
    nk, nu = len(p["morphs"]), len(p["unk_morphs"])

    def rc_of(spec):
        return word_table(known, unk, nk, nu, spec)[0]

    ok, keep = make_spec(1, W.KEEP, ("名詞",), ord("|"))
    rc, _, _, sep = word_table(known, unk, nk, nu, ok)
    assert rc == _lib.KGPU_OK and sep == ord("|")
    bad = _lib.KGPU_ERR_INVALID_ARG
    assert L.kgpu_debug_word_table(None, 0, None, 0, 0, 0, None, None, None, 0, None, None) == bad   # a null spec
    assert rc_of(make_spec(size=C.sizeof(_lib.WordsSpec) - 1)[0]) == bad
    assert rc_of(make_spec(size=0)[0]) == bad
    assert rc_of(make_spec(size=C.sizeof(_lib.WordsSpec) + 8)[0]) == _lib.KGPU_OK   # a later, longer struct
    assert rc_of(make_spec(field=-2)[0]) == bad
    assert rc_of(make_spec(filt=3)[0]) == bad
    assert rc_of(make_spec(separator=256)[0]) == bad
    assert rc_of(make_spec(separator=10)[0]) == bad
    assert rc_of(make_spec(separator=255)[0]) == _lib.KGPU_OK
    s, keep = make_spec(names=("名詞",))
    s.name_offsets = None
    assert rc_of(s) == bad                                   # names without offsets
    s, keep = make_spec(names=("名詞", "助詞"))
    keep[1][1] = 99
    assert rc_of(s) == bad                                   # offsets that run backwards
    s, keep = make_spec(names=("名詞",))
    s.names = None
    assert rc_of(s) == bad                                   # offsets without names
    s, keep = make_spec(filt=W.KEEP, names=())
    s.names = None
    assert rc_of(s) == _lib.KGPU_OK                          # an empty list is legal
    # null pointers of kgpu_words_create itself: rejected before a dictionary is touched
    out = C.c_void_p()
    assert L.kgpu_words_create(None, C.byref(ok), C.byref(out)) == bad
    assert L.kgpu_tokenize_batch_words(None, None, None, 0, None, 0, None, None, None) == bad
    assert L.kgpu_tokenize_text_words(None, None, 0, None, 0, None, 0, None, None, None) == bad
    assert L.kgpu_format_words_device(None, None, None, None, 0, None, None, None, 0, None) == bad
    L.kgpu_words_destroy(None)


def test_python_spec_checks():
    from kanpyo_amd.tokenizer import words_spec

    spec, keep = words_spec(field=7, drop=["助詞", "記号"], separator="|")
    assert (spec.size, spec.field, spec.filter, spec.separator, spec.n_names) == (C.sizeof(_lib.WordsSpec), 7, _lib.KGPU_WORDS_DROP, ord("|"), 2)
    assert keep[0].tobytes() == "助詞記号".encode() and keep[1].tolist() == [0, 6, 12]
    spec, _ = words_spec()
    assert (spec.field, spec.filter, spec.separator, spec.n_names) == (-1, _lib.KGPU_WORDS_ALL, 32, 0)
    assert words_spec(keep=["感動詞"])[0].filter == _lib.KGPU_WORDS_KEEP
    for kw in ({"drop": ["a"], "keep": ["b"]}, {"separator": "ab"}, {"separator": ""}, {"separator": "あ"}):
        with pytest.raises(ValueError):
            words_spec(**kw)


def test_cli_argument_parsing():
    from kanpyo_amd import cli

    a = cli.parse_args(["wakati"])
    assert (a.command, a.input, a.field, a.drop, a.keep, a.separator, a.split) == ("wakati", None, None, [], [], " ", "host")
    a = cli.parse_args(["wakati", "すもも", "-c", "x.dict", "--reading", "--drop", "助詞,助動詞,記号", "--separator", "|", "--split", "device"])
    assert (a.input, a.custom_dict, a.field, a.drop, a.keep, a.separator, a.split) == ("すもも", "x.dict", 7, ["助詞", "助動詞", "記号"], [], "|", "device")
    assert cli.parse_args(["wakati", "--base-form"]).field == 6 and cli.parse_args(["wakati", "--pronunciation"]).field == 8
    assert cli.parse_args(["wakati", "--field", "0", "--keep", "名詞"]).keep == ["名詞"]
    for argv in (["wakati", "--field", "3", "--reading"], ["wakati", "--drop", "a", "--keep", "b"], ["wakati", "--field", "-1"], ["wakati", "--field", "x"],
                 ["wakati", "--separator", "ab"], ["wakati", "--separator", "\n"], ["wakati", "--separator", ""], ["wakati", "--split", "gpu"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    # the reference's own command line is what it was
    assert cli.parse_args([]).command == "tokenize" and cli.parse_args(["graphviz", "-f"]).full_state


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in ("kgpu_words_create", "kgpu_words_destroy", "kgpu_tokenize_batch_words", "kgpu_tokenize_text_words", "kgpu_format_words_device"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert hasattr(L, "kgpu_debug_word_table")


def test_words_consumer_is_strict_c99_and_links(tmp_path):
    exe = str(tmp_path / "words_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "words_consumer.c"), "-o", exe,
                    "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    syms = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    used = {w for line in syms.splitlines() for w in line.split() if w.startswith("kgpu_")}
    assert {"kgpu_words_create", "kgpu_words_destroy", "kgpu_tokenize_batch_words", "kgpu_tokenize_text_words"} <= used


def test_words_spec_layout_matches_the_ctypes_mirror(tmp_path):
    exe = str(tmp_path / "words_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "words_layout.c"), "-o", exe], check=True)
    fields, consts = {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, a, b = line.split()
        if st == "const":
            consts[f] = int(a)
        else:
            assert st == "kgpu_words_spec"
            fields[f] = (int(a), int(b))
    assert fields.pop("-") == (0, C.sizeof(_lib.WordsSpec))
    assert set(fields) == {n for n, _ in _lib.WordsSpec._fields_}
    for f, (off, size) in fields.items():
        m = getattr(_lib.WordsSpec, f)
        assert (m.offset, m.size) == (off, size), f
    assert consts == {"KGPU_WORDS_SURFACE": _lib.KGPU_WORDS_SURFACE, "KGPU_WORDS_ALL": _lib.KGPU_WORDS_ALL, "KGPU_WORDS_DROP": _lib.KGPU_WORDS_DROP,
                      "KGPU_WORDS_KEEP": _lib.KGPU_WORDS_KEEP}
