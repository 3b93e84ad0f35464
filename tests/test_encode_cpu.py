"""The host side of the vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids") without a device: tests/encode_ref.py against the hand-derived
tests/golden/fixture_encode.json; the invariant that encode and count agree on a word's identity; the handle's two tables through the
kgpu_debug_vocab_table hook against the reference's row ids, its hash and a Python probe; the table builder alone under AddressSanitizer + UBSan
as a stand-alone program; the new symbols; the C layout of the new structs; the CLI's argument parsing."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import count_ref as CR
import encode_ref as E
import words_ref as W
from conftest import ROOT, load_golden
from golden_cases import fixture_tables, golden_records, synth20k, vocab_table  # noqa: F401  (synth20k: the fixture)
from kanpyo_amd import _lib
from record_cases import ref_spec

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
NEW = ("kgpu_vocab_create", "kgpu_vocab_destroy", "kgpu_vocab_get_info", "kgpu_encode_batch", "kgpu_encode_text", "kgpu_encode_device")
SPECS = {   # tests/test_gpu_words.py's (restated: that module is a GPU module)
    "surface": {}, "field0": {"field": 0}, "field7": {"field": 7}, "field8": {"field": 8}, "field40": {"field": 40},
    "drop": {"drop": ("助詞", "助動詞", "記号")}, "keep": {"keep": ("感動詞",)},
}


def test_reference_reproduces_the_golden_ids():
    p, known, unk = fixture_tables()
    cases = load_golden("fixture_encode.json")["cases"]
    assert len(cases) >= 5
    assert any(c["unk_id"] in sum(c["ids"], []) for c in cases), "the golden needs a word outside the list"
    assert any(c["bos_id"] is not None and c["eos_id"] is not None for c in cases) and any("" in c["sentences"] for c in cases)
    for c in cases:
        spec = W.Spec(c["field"], c["filter"], c["names"])
        ids, off = E.encode(*golden_records(c["sentences"]), known, unk, len(p["morphs"]), len(p["unk_morphs"]), spec, p["sorted_keywords"],
                            c["vocab"], c["unk_id"], c["bos_id"], c["eos_id"])
        assert ids.dtype == np.int32 and off.dtype == np.uint64
        assert [ids[int(off[i]) : int(off[i + 1])].tolist() for i in range(len(off) - 1)] == c["ids"], c
    with pytest.raises(ValueError):
        E.encode_words([[b"a"]], ["a", "b", "a"], 0)
    assert E.padded(np.array([5, 6, 7, 8, 9], dtype=np.int32), [0, 3, 3, 5], 2, -1, eos_id=4).tolist() == [[5, 4], [-1, -1], [8, 9]]
    assert E.padded(np.array([5, 6, 7], dtype=np.int32), [0, 3], 2, -1).tolist() == [[5, 6]]


def test_encode_and_count_agree_on_identity(synth20k):
    """Over 2000 cfg 2 sentences with the oracle's tokens: with the whole read-out as the list, the words of the ids are the counts; with
    min_count = 2 the unk ids are the singleton words' tokens."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    sd, known, unk, nk, nu, keys = synth20k
    utf8, offs = pack_sentences(synth.make_corpus(sd, 2000, 3, "cfg2"))
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 1)
    for name in ("surface", "field7", "drop"):
        spec = ref_spec(**SPECS[name])
        counts = CR.count(utf8, offs, exp.tokens, exp.offsets, known, unk, nk, nu, spec, keys, own_records=True)
        vocab = [w for w, _ in CR.ordered(counts)]
        ids, off = E.encode(utf8, offs, exp.tokens, exp.offsets, known, unk, nk, nu, spec, keys, vocab, -1)
        assert int(off[-1]) == len(ids) == sum(counts.values()) and -1 not in ids
        assert Counter(vocab[i] for i in ids.tolist()) == counts, name
        assert np.array_equal(np.bincount(ids, minlength=len(vocab)), [n for _, n in CR.ordered(counts)])
        kept = [w for w, n in CR.ordered(counts) if n >= 2]
        singles = sum(n for n in counts.values() if n == 1)
        assert 0 < singles < sum(counts.values())
        ids2, _ = E.encode(utf8, offs, exp.tokens, exp.offsets, known, unk, nk, nu, spec, keys, ["<pad>", "<unk>"] + kept, 1)
        assert int((ids2 == 1).sum()) == singles and 0 not in ids2, name


# ---- the handle's tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPECS))
def test_vocab_table_on_the_synthetic_dictionary(synth20k, name):
    sd, known, unk, nk, nu, keys = synth20k
    kw = SPECS[name]
    spec = ref_spec(**kw)
    # the list: every second word the rows can give, and strangers of several shapes (the empty word among them)
    row_words = sorted({w for w in (W.row_word(t.features(i), spec) for t, n in ((known, nk), (unk, nu)) for i in range(1, n + 1)) if w is not None}
                       | {k.encode() for k in keys})
    vocab = [b"<pad>", b"<unk>", b""] + row_words[::2] + [b"stranger-%d" % i for i in range(300)] + [bytes([i % 255 + 1]) * (i % 40 + 1) + b"\0" for i in range(200)]
    assert len(set(vocab)) == len(vocab)
    rc, row_id, slots, arena, resolved = vocab_table(sd.dict, known, unk, nk, nu, kw, vocab, 1)
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    want = E.row_ids(known, unk, nk, nu, spec, keys, vocab, 1)
    read = [i for i, w in enumerate(want) if w is not None]
    assert len(read) >= nk and np.array_equal(row_id[read], [want[i] for i in read]), name
    listed = sum(1 for i in read if want[i] != 1)
    assert resolved == listed and 0 < listed < len(read), (resolved, listed)
    n = len(slots)
    assert n & (n - 1) == 0 and n >= 2 * len(vocab) and n >= 16
    used = np.flatnonzero(slots[:, 0])
    assert len(used) == len(vocab)
    for i in used.tolist():   # every slot's tag carries the reference hash of its entry's bytes
        tag = int(slots[i][0])
        at = ((tag & 0xFFFFFFFF) - 1) * 8
        length = int.from_bytes(arena[at : at + 4], "little")
        word = arena[at + 8 : at + 8 + length]
        assert tag >> 32 == E.key_hash(word) == int.from_bytes(arena[at + 4 : at + 8], "little") and vocab[int(slots[i][1])] == word
    far = 0
    for k, w in enumerate(vocab):   # every list word is found by a Python probe of the returned slots
        got, steps = E.probe(slots, arena, w)
        assert got == k, (k, w)
        far = max(far, steps)
    assert far >= 2, "no word sits two slots or more from its home: the probe's walk is not exercised"
    for w in (b"stranger-300", b"stranger-1\0", b"<pad", b"\0", row_words[1] + b"x"):
        assert E.probe(slots, arena, w)[0] is None


def test_vocab_table_duplicates_empty_word_and_errors(synth20k):
    sd, known, unk, nk, nu, keys = synth20k
    bad = _lib.KGPU_ERR_INVALID_ARG
    rc, *_ = vocab_table(sd.dict, known, unk, nk, nu, {}, [b"a", b"b", b"c", b"b"], 0)
    msg = _lib.lib().kgpu_last_error().decode()
    assert rc == bad and " 1 " in msg and " 3 " in msg, msg
    rc, *_ = vocab_table(sd.dict, known, unk, nk, nu, {}, [b"", b"x", b""], 0)
    assert rc == bad and " 0 " in _lib.lib().kgpu_last_error().decode() and " 2 " in _lib.lib().kgpu_last_error().decode()
    rc, row_id, slots, arena, resolved = vocab_table(sd.dict, known, unk, nk, nu, {}, [b"x", b""], -9)   # the empty word is accepted
    assert rc == _lib.KGPU_OK and E.probe(slots, arena, b"") == (1, 0) and len(slots) == 16 and resolved == 0 and (row_id[:nk] == -9).all()
    rc, row_id, slots, arena, resolved = vocab_table(sd.dict, known, unk, nk, nu, {}, [], 7)                # ... and so is the empty list
    assert rc == _lib.KGPU_OK and len(slots) == 16 and not slots.any() and (row_id[:nk] == 7).all()
    assert vocab_table(sd.dict, known, unk, nk, nu, {}, [b"a"], 0, flags=4)[0] == bad                          # unknown flags
    L = _lib.lib()
    out, ne = C.c_void_p(), C.c_uint64(0)
    opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), 0, 0, 0, 0)
    assert L.kgpu_vocab_create(None, None, None, 0, C.byref(opts), C.byref(out)) == bad and L.kgpu_vocab_get_info(None, None) == bad
    assert L.kgpu_encode_batch(None, None, None, 0, None, 0, None, None, C.byref(ne)) == bad
    assert L.kgpu_encode_text(None, None, 0, None, 0, None, 0, None, C.byref(ne), C.byref(ne)) == bad
    assert L.kgpu_encode_device(None, None, None, None, 0, None, None, None, 0, 0, 0, None) == bad
    L.kgpu_vocab_destroy(None)


def test_table_builder_alone_under_asan_ubsan(tmp_path):
    """kgpu_vocab_table.cpp and tests/c_abi/vocab_table_main.cpp (its own main), built by plain g++ with the sanitizers (their runtimes linked statically) and run as a program."""
    exe = str(tmp_path / "vocab_table_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-omit-frame-pointer", os.path.join(HERE, "vocab_table_main.cpp"), os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_vocab_table.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes are linked statically)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "vocab table ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes, s
    assert hasattr(L, "kgpu_debug_vocab_table") and "kgpu_debug_vocab_table" not in _lib.SYMBOLS
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    assert "kgpu_debug_vocab_table" not in header and all(s + "(" in header for s in NEW)
    assert header.index("vocabulary ids") > header.index("word counts")


def test_vocab_structs_layout_matches_the_ctypes_mirrors(tmp_path):
    exe = str(tmp_path / "encode_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "encode_layout.c"), "-o", exe], check=True)
    fields, consts = {"kgpu_vocab_opts": {}, "kgpu_vocab_info": {}}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, a, b = line.split()
        if st == "const":
            consts[f] = int(a)
        else:
            fields[st][f] = (int(a), int(b))
    for name, mirror in (("kgpu_vocab_opts", _lib.VocabOpts), ("kgpu_vocab_info", _lib.VocabInfo)):
        got = fields[name]
        assert got.pop("-") == (0, C.sizeof(mirror))
        assert set(got) == {n for n, _ in mirror._fields_}
        for f, (off, size) in got.items():
            m = getattr(mirror, f)
            assert (m.offset, m.size) == (off, size), (name, f)
    assert C.sizeof(_lib.VocabOpts) == 20 and C.sizeof(_lib.VocabInfo) == 40
    assert consts == {"KGPU_VOCAB_ADD_BOS": _lib.KGPU_VOCAB_ADD_BOS, "KGPU_VOCAB_ADD_EOS": _lib.KGPU_VOCAB_ADD_EOS} and consts["KGPU_VOCAB_ADD_EOS"] == 2


def test_encode_consumer_is_strict_c99_and_links(tmp_path):
    exe = str(tmp_path / "encode_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "encode_consumer.c"), "-o", exe,
                    "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    syms = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    used = {w for line in syms.splitlines() for w in line.split() if w.startswith("kgpu_")}
    assert {"kgpu_vocab_create", "kgpu_vocab_destroy", "kgpu_vocab_get_info", "kgpu_encode_batch", "kgpu_encode_text"} <= used


def test_vocab_file_round_trip(tmp_path):
    from kanpyo_amd.vocab import Vocab

    v = Vocab.__new__(Vocab)   # (the file format alone: no handle, no device)
    v.words = [b"<pad>", b"<unk>", b"", "辞書".encode(), b"a b\tc", b"\xff\xfe"]
    path = tmp_path / "v.txt"
    Vocab.save(v, path)
    assert path.read_bytes() == b"<pad>\n<unk>\n\n" + "辞書".encode() + b"\na b\tc\n\xff\xfe\n" and Vocab.read_words(path) == v.words
    v.words = [b"ok", b"two\nlines"]
    with pytest.raises(ValueError):
        Vocab.save(v, path)
    v._h = v._ctx = None


def test_cli_argument_parsing():
    from kanpyo_amd import cli

    a = cli.parse_args(["encode", "--vocab", "v.txt"])
    assert (a.command, a.input, a.vocab, a.field, a.drop, a.keep, a.unk, a.bos, a.eos, a.split, a.skip_invalid) == \
        ("encode", None, "v.txt", None, [], [], "<unk>", None, None, "host", False)
    a = cli.parse_args(["encode", "すもも", "-c", "x.dict", "--vocab", "v", "--reading", "--drop", "助詞,記号", "--unk", "U", "--bos", "<s>", "--eos", "</s>",
                        "--split", "device", "--skip-invalid"])
    assert (a.input, a.custom_dict, a.field, a.drop, a.unk, a.bos, a.eos, a.split, a.skip_invalid) == ("すもも", "x.dict", 7, ["助詞", "記号"], "U", "<s>", "</s>", "device", True)
    for argv in (["encode"], ["encode", "--vocab", "v", "--field", "3", "--reading"], ["encode", "--vocab", "v", "--drop", "a", "--keep", "b"],
                 ["encode", "--vocab", "v", "--split", "gpu"], ["encode", "--vocab", "v", "--separator", "|"], ["encode", "--vocab", "v", "--top", "3"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    assert cli.parse_args([]).command == "tokenize" and cli.parse_args(["count", "--top", "3"]).top == 3 and not hasattr(cli.parse_args(["count"]), "vocab")
