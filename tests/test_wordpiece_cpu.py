"""The host side of the WordPiece ids (include/kanpyo_gpu.h, "WordPiece ids") without a device: tests/wordpiece_ref.py against the hand-derived
tests/golden/fixture_wordpiece.json and, where `tokenizers` is installed, against tokenizers.models.WordPiece; the library's host split
(kgpu_debug_wordpiece_split) and every row entry of a handle's tables (kgpu_debug_wordpiece_table) against the reference; both byte tables probed
in Python; colliding keys and a wrapped chain in the CONTINUATION table; the cases of tests/wordpiece_cases.py (what the device tests of
tests/test_gpu_wordpiece_adversarial.py run) through the host split; the table builder under AddressSanitizer + UBSan as a stand-alone program;
the new symbols, the C layout of the new structs, the argument errors and the CLI's argument parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encode_ref as E
import table_keys as TK
import wordpiece_cases as WC
import wordpiece_ref as WP
import words_ref as W
from conftest import ROOT, load_golden
from kanpyo_amd import _lib
from record_cases import characters, ref_spec

HERE = os.path.join(ROOT, "tests", "c_abi")
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "kanpyo_amd", "csrc")
NEW = ("kgpu_vocab_create_wordpiece", "kgpu_vocab_get_wordpiece_info")


def lib_split(vocab, words, unk_id, prefix=b"##", max_chars=100):
    from kanpyo_amd.vocab import split_words, wordpiece_opts

    return [a.tolist() for a in split_words(vocab, words, unk_id, wordpiece_opts(prefix, max_chars))]


def golden_cases():
    for c in load_golden("fixture_wordpiece.json")["cases"]:
        vocab = [WP.golden_bytes(x) for x in c["list"]]
        yield c, vocab, vocab.index(WP.golden_bytes(c["unk"])), WP.golden_bytes(c["prefix"])


def test_reference_and_host_split_reproduce_the_golden_pieces():
    names, n_words = set(), 0
    for c, vocab, unk, prefix in golden_cases():
        names.add(c["name"])
        words = [WP.golden_bytes(w["word"]) for w in c["words"]]
        want = [[vocab.index(p) for p in WP.golden_pieces(w["pieces"])] for w in c["words"]]
        assert [WP.split(w, vocab, prefix, c["max_chars"], unk) for w in words] == want, c["name"]
        assert lib_split(vocab, words, unk, prefix, c["max_chars"]) == want, c["name"]
        n_words += len(words)
    assert len(names) >= 7 and n_words >= 30
    first = next(golden_cases())
    by_word = {WP.golden_bytes(w["word"]): [p if isinstance(p, str) else p for p in w["pieces"]] for w in first[0]["words"]}
    assert by_word["あいうえお".encode()] == ["あ", "##い", "##う", "##えお"] and by_word["あいうえおか".encode()] == ["[UNK]"] and by_word[b""] == []
    assert by_word["あ".encode() * 101] == ["[UNK]"] and by_word[b"##abc"] == ["##abc"] and by_word[b"##"] == ["##"]
    assert any(c["prefix"] == "" for c, *_ in golden_cases()) and any(len(WP.golden_pieces(w["pieces"])) == 100 for c, *_ in golden_cases() for w in c["words"])
    with pytest.raises(ValueError):
        WP.tables([b"a", b"b", b"a"])


def test_reference_against_tokenizers_wordpiece():
    """The external pin: a few thousand random words over a small alphabet and a random list, through tokenizers.models.WordPiece."""
    tokenizers = pytest.importorskip("tokenizers")
    rng = np.random.default_rng(3)
    alphabet = ["a", "b", "c", "é", "あ", "い", "ス", "𠮷"]
    word = lambda n: "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))   # noqa: E731
    for prefix, max_chars in (("##", 100), ("##", 6), ("@", 100)):
        vocab = ["[UNK]"]
        for _ in range(150):
            w = word(int(rng.integers(1, 4)))
            w = prefix + w if rng.integers(0, 2) else w
            if w not in vocab:
                vocab.append(w)
        model = tokenizers.models.WordPiece({w: k for k, w in enumerate(vocab)}, unk_token="[UNK]", max_input_chars_per_word=max_chars, continuing_subword_prefix=prefix)
        words = [word(int(rng.integers(1, 10))) for _ in range(1500)]
        want = [[t.id for t in model.tokenize(w)] for w in words]
        got = [WP.split(w, vocab, prefix, max_chars, 0) for w in words]
        assert got == want, (prefix, max_chars)
        assert sum(len(g) > 1 for g in got) > 100 and sum(g == [0] for g in got) > 100 and sum(len(g) == 1 and g != [0] for g in got) > 5
        assert lib_split(vocab, words, 0, prefix, max_chars) == want


# ---- the handle's tables -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth20k():
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    return sd, known, unk, len(known.morph_features), len(unk.morph_features), synth.record_surfaces(sd)


def wordpiece_table(sd_dict, known, unk, nk, nu, kw, words, unk_id, prefix=b"##", max_chars=100, wp=None):
    """kgpu_debug_wordpiece_table -> (rc, {"initial": (slots, arena), "cont": (slots, arena), "rows": uint32 [n, 2], "pool": int32, "info": dict})."""
    from kanpyo_amd._calls import struct_dict
    from kanpyo_amd.tokenizer import pack_sentences, words_spec
    from kanpyo_amd.vocab import wordpiece_opts

    L = _lib.lib()
    spec, keep = words_spec(**kw)
    kb = np.frombuffer(known.encode(), dtype=np.uint8)
    ub = np.frombuffer(unk.encode(), dtype=np.uint8)
    ib = np.frombuffer(sd_dict.index_dict, dtype=np.uint8)
    packed, woff = pack_sentences(words)
    packed = np.ascontiguousarray(packed)
    opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), 0, unk_id, 0, 0)
    wp = wordpiece_opts(prefix, max_chars) if wp is None else wp
    info = _lib.WordpieceInfo(C.sizeof(_lib.WordpieceInfo))
    sizes = np.zeros(6, dtype=np.uint64)
    head = (kb.ctypes.data, kb.size, ub.ctypes.data, ub.size, ib.ctypes.data, ib.size, nk, nu, C.byref(spec), packed.ctypes.data if packed.size else None,
            woff.ctypes.data, len(words), C.byref(opts), C.byref(wp) if wp is not False else None, sizes.ctypes.data)
    rc = L.kgpu_debug_wordpiece_table(*head, None, None, None, None, None, None, C.byref(info))
    if rc != _lib.KGPU_ERR_CAPACITY:
        return rc, None
    n = [int(x) for x in sizes]
    islots, cslots = np.zeros((n[0], 2), dtype=np.uint64), np.zeros((n[2], 2), dtype=np.uint64)
    iarena, carena = np.zeros(max(n[1], 1), dtype=np.uint8), np.zeros(max(n[3], 1), dtype=np.uint8)
    rows, pool = np.zeros((max(n[4], 1), 2), dtype=np.uint32), np.zeros(max(n[5], 1), dtype=np.int32)
    rc = L.kgpu_debug_wordpiece_table(*head, islots.ctypes.data, iarena.ctypes.data, cslots.ctypes.data, carena.ctypes.data, rows.ctypes.data, pool.ctypes.data, C.byref(info))
    del keep
    assert [int(x) for x in sizes] == n
    return rc, {"initial": (islots, iarena.tobytes()[: n[1]]), "cont": (cslots, carena.tobytes()[: n[3]]), "rows": rows[: n[4]], "pool": pool[: n[5]],
                "info": struct_dict(info)}


def row_pieces(t, r):
    first, count = int(t["rows"][r][0]), int(t["rows"][r][1])
    if count == 1:
        return [int(np.int32(np.uint32(first)))]
    return t["pool"][first : first + count].tolist()


@pytest.mark.parametrize("name, kw", [("surface", {}), ("field7", {"field": 7}), ("drop", {"drop": ("助詞", "助動詞", "記号")})])
def test_wordpiece_table_on_the_synthetic_dictionary(synth20k, name, kw):
    sd, known, unk, nk, nu, keys = synth20k
    spec = ref_spec(**kw)
    row_words = sorted({w for w in (W.row_word(t.features(i), spec) for t, n in ((known, nk), (unk, nu)) for i in range(1, n + 1)) if w is not None}
                       | {k.encode() for k in keys})
    chars = characters(row_words)
    left_out = set(chars[5::40])   # a handful of characters with no entry at all: their words give [UNK] unless listed whole
    vocab = [b"[PAD]", b"[UNK]", b""] + row_words[::3] + [c for c in chars if c not in left_out and c not in set(row_words[::3])] + [b"##" + c for c in chars if c not in left_out]
    assert len(set(vocab)) == len(vocab) and left_out
    rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, kw, vocab, 1)
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    want = WP.rows(known, unk, nk, nu, spec, keys, vocab, 1)
    read = [r for r, w in enumerate(want) if w is not None]
    assert len(read) >= nk and len(t["rows"]) == nk + nu
    listed = set(vocab)
    whole = split = unks = pooled = 0
    for r in read:
        assert row_pieces(t, r) == want[r], (name, r)
        if len(want[r]) != 1:
            pooled += len(want[r])
    for r, w in enumerate(want):   # the outcome counters, by the reference
        if w is None:
            continue
        word = W.row_word((known if r < nk else unk).features(r + 1 if r < nk else r - nk + 1), spec)
        word = keys[r].encode() if word is None else word
        whole += len(w) == 1 and word in listed
        split += len(w) > 1
        unks += len(w) == 1 and word not in listed
    info = t["info"]
    assert (info["rows_whole"], info["rows_split"], info["rows_unk"], info["row_piece_ids"]) == (whole, split, unks, pooled), name
    assert whole > 100 and split > 100 and unks > 10, "rows of every outcome"
    cont = [w[2:] for w in vocab if w.startswith(b"##") and len(w) > 2]
    assert info["cont_words"] == len(cont) and info["max_initial_bytes"] == max(map(len, vocab)) and info["max_cont_bytes"] == max(map(len, cont))
    # both byte tables, probed in Python
    islots, iarena = t["initial"]
    cslots, carena = t["cont"]
    for slots, n_entries in ((islots, len(vocab)), (cslots, len(cont))):
        n = len(slots)
        assert n & (n - 1) == 0 and n >= 2 * n_entries and n >= 16 and len(np.flatnonzero(slots[:, 0])) == n_entries
    assert info["cont_table_slots"] == len(cslots) and info["cont_key_bytes"] == len(carena)
    for k, w in enumerate(vocab):
        assert E.probe(islots, iarena, w)[0] == k
        if w.startswith(b"##") and len(w) > 2:
            assert E.probe(cslots, carena, w[2:])[0] == k and E.probe(cslots, carena, w)[0] is None
        else:
            hit = E.probe(cslots, carena, w)[0]
            assert hit is None or vocab[hit] == b"##" + w
    # the host split on the same words
    sample = row_words[::7] + [b"", chars[5] * 3, row_words[1] + row_words[2]]
    tabs = WP.tables(vocab)
    assert lib_split(vocab, sample, 1) == [WP.split_with(tabs, w, 100, 1) for w in sample]


def test_prefix_of_no_bytes_shares_one_table(synth20k):
    sd, known, unk, nk, nu, keys = synth20k
    vocab = [b"[UNK]"] + [k.encode() for k in keys[:400]] + characters([k.encode() for k in keys[:2000]])
    vocab = list(dict.fromkeys(vocab))
    rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0, prefix=b"")
    assert rc == _lib.KGPU_OK
    assert t["info"]["cont_words"] == len(vocab) and t["info"]["cont_table_slots"] == len(t["initial"][0]) and t["info"]["max_cont_bytes"] == t["info"]["max_initial_bytes"]
    assert np.array_equal(t["cont"][0], t["initial"][0]) and t["cont"][1] == t["initial"][1]
    want = WP.rows(known, unk, nk, nu, ref_spec(), keys, vocab, 0, prefix=b"")
    assert all(row_pieces(t, r) == w for r, w in enumerate(want) if w is not None) and t["info"]["rows_split"] > 100


def test_colliding_keys_and_a_wrapped_chain_in_the_continuation_table(synth20k):
    sd, known, unk, nk, nu, keys = synth20k
    lead = lambda k: k[0] & 0xC0 != 0x80   # noqa: E731  (a piece starts at a character start: keys whose first byte is 10xxxxxx cannot follow "X")
    same, cross, _ = TK.adversarial_pairs()
    pairs = [(a, b) for a, b in same + cross if lead(a) and lead(b)]
    assert len(pairs) >= 4 and all(E.key_hash(a) == E.key_hash(b) and a != b for a, b in pairs)
    for which in ("both", "first", "second"):
        vocab = [b"[UNK]", b"X"] + [b"##" + k for a, b in pairs for k in ((a, b) if which == "both" else (a,) if which == "first" else (b,))]
        words = [b"X" + k for pr in pairs for k in pr] + [b"X" + a + b for a, b in pairs] + [a for a, _ in pairs]
        tabs = WP.tables(vocab)
        want = [WP.split_with(tabs, w, 100, 0) for w in words]
        assert sum(len(w) == 2 for w in want) >= (2 if which == "both" else 1) * len(pairs) and (which == "both" or sum(w == [0] for w in want) >= len(pairs))
        assert lib_split(vocab, words, 0) == want, which
        rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0)
        assert rc == _lib.KGPU_OK
        for k, w in enumerate(vocab[2:], 2):
            assert E.probe(*t["cont"], w[2:])[0] == k
        if which != "both":
            absent = [b if which == "first" else a for a, b in pairs]
            assert all(E.probe(*t["cont"], k)[0] is None for k in absent)
    # eight continuation entries whose home is the last of 16 slots: the chain wraps round the table's end
    chain, absent15, covered = TK.chain(16, 15, 8)
    assert all(E.key_hash(k) & 15 == 15 for k in chain + absent15)
    ok = [k for k in chain + absent15 + covered if lead(k)]
    vocab = [b"[UNK]", b"X"] + [b"##" + k for k in chain]
    rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0)
    cslots, carena = t["cont"]
    assert rc == _lib.KGPU_OK and len(cslots) == 16 and len(t["initial"][0]) == 32
    assert [int(cslots[i][1]) if cslots[i][0] else None for i in (15, 0, 1, 2, 3, 4, 5, 6, 7)] == [2, 3, 4, 5, 6, 7, 8, 9, None]
    assert [E.probe(cslots, carena, k) for k in chain] == [(k + 2, k) for k in range(8)]
    assert all(E.probe(cslots, carena, k) == (None, 8) for k in absent15)
    words = [b"X" + k for k in ok] + [b"X" + chain[7] + chain[0]] * lead(chain[7]) * lead(chain[0])
    tabs = WP.tables(vocab)
    want = [WP.split_with(tabs, w, 100, 0) for w in words]
    assert any(len(w) == 2 for w in want) and [0] in want
    assert lib_split(vocab, words, 0) == want


# ---- the cases of tests/test_gpu_wordpiece_adversarial.py through the HOST split: a disagreement shows on a machine without a GPU first -------------------------
def host_agrees(case, words=None):
    """kgpu_debug_wordpiece_split on the case's distinct words (or `words`) against wordpiece_ref, word for word."""
    sp = case.split()
    words = case.words() if words is None else words
    tabs = case.tables()
    want = [sp[w] if w in sp else WP.split_with(tabs, w, case.max_chars, WC.UNK) for w in words]
    got = lib_split(case.vocab, words, WC.UNK, case.prefix, case.max_chars)
    assert got == want, (case, next((w[:40], g[:8], x[:8]) for w, g, x in zip(words, got, want) if g != x))


def test_host_split_on_colliding_prefixes():
    for case, trios in WC.twin_cases():
        WC.claim_twin(case, trios)
        host_agrees(case)
    case, pairs = WC.both_listed_case()
    WC.claim_both_listed(case, pairs)
    host_agrees(case)
    for case, asked in WC.cross_length_cases():
        WC.claim_cross(case, asked)
        host_agrees(case)
    for case, keys in WC.both_tables_cases():
        WC.claim_both_tables(case, keys)
        host_agrees(case)
    one, rotated, keys = WC.chain_cases()
    WC.claim_chain(one, rotated, keys)
    host_agrees(one)
    host_agrees(rotated)


def test_host_split_at_the_tables_longest_entries():
    for case in WC.longest_entry_cases():
        WC.claim_longest(case)
        host_agrees(case)


@pytest.mark.parametrize("limit", WC.LIMITS)
def test_host_split_at_max_word_chars(limit):
    case, count = WC.limit_case(limit)
    WC.claim_limit(case, count, limit)
    host_agrees(case)
    if limit == 1024:
        WC.claim_full_window(WC.full_window_case())
        host_agrees(WC.full_window_case())


@pytest.mark.parametrize("limit", WC.RANDOM_LIMITS)
@pytest.mark.parametrize("prefix", WC.PREFIXES, ids=["hashes", "at", "none", "eight-bytes"])
def test_host_split_on_random_lists(prefix, limit):
    """test_reference_against_tokenizers_wordpiece's draw, with the conditions asserted by the reference for every (prefix, limit), and the words of the
    shifted layout: records that start inside a character, so the word begins with 10xxxxxx bytes -- "a character starts at byte 0"."""
    case = WC.random_case(prefix, limit)
    WC.claim_random(case)
    assert len(prefix) in (0, 1, 2, 8)
    host_agrees(case)
    shifted = list(dict.fromkeys(w for s in WC.record_words(WC.records(case.sentences, shift=True)) for w in s))
    inside = [w for w in shifted if w and w[0] & 0xC0 == 0x80]
    assert len(inside) >= 100, "words that begin inside a character"
    tabs = case.tables()
    assert all(WP.split_with(tabs, w, limit, WC.UNK) == [WC.UNK] for w in inside), "by the reference: the first character is the stray bytes, which no list holds"
    host_agrees(case, shifted)


def test_table_builder_alone_under_asan_ubsan(tmp_path):
    """kgpu_wordpiece_table.cpp, kgpu_vocab_table.cpp and tests/c_abi/wordpiece_table_main.cpp (its own main), built by plain g++ with the sanitizers (their
    runtimes linked statically) and run as a program."""
    exe = str(tmp_path / "wordpiece_table_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-omit-frame-pointer", os.path.join(HERE, "wordpiece_table_main.cpp"), os.path.join(CSRC, "kgpu_wordpiece_table.cpp"),
                        os.path.join(CSRC, "kgpu_vocab_table.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")   # (the runtimes are linked statically)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wordpiece table ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes, s
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    for s in ("kgpu_debug_wordpiece_table", "kgpu_debug_wordpiece_split"):
        assert hasattr(L, s) and s not in _lib.SYMBOLS and s not in header
    assert all(s + "(" in header for s in NEW) and header.index("WordPiece ids") > header.index("vocabulary ids")


def test_wordpiece_structs_layout_matches_the_ctypes_mirrors(tmp_path):
    exe = str(tmp_path / "wordpiece_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, os.path.join(HERE, "wordpiece_layout.c"), "-o", exe], check=True)
    fields = {"kgpu_wordpiece_opts": {}, "kgpu_wordpiece_info": {}}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        st, f, a, b = line.split()
        fields[st][f] = (int(a), int(b))
    for name, mirror in (("kgpu_wordpiece_opts", _lib.WordpieceOpts), ("kgpu_wordpiece_info", _lib.WordpieceInfo)):
        got = fields[name]
        assert got.pop("-") == (0, C.sizeof(mirror))
        assert set(got) == {n for n, _ in mirror._fields_}
        for f, (off, size) in got.items():
            m = getattr(mirror, f)
            assert (m.offset, m.size) == (off, size), (name, f)
    assert C.sizeof(_lib.WordpieceOpts) == 20 and C.sizeof(_lib.WordpieceInfo) == 80
    assert C.sizeof(_lib.VocabOpts) == 20 and C.sizeof(_lib.VocabInfo) == 40, "the plain vocabulary's structs are untouched"


def test_argument_errors(synth20k):
    sd, known, unk, nk, nu, keys = synth20k
    bad = _lib.KGPU_ERR_INVALID_ARG
    L = _lib.lib()
    mk = lambda size, chars, plen: _lib.WordpieceOpts(size, chars, plen, (C.c_uint8 * 8)(*b"##"))   # noqa: E731
    full = C.sizeof(_lib.WordpieceOpts)
    vocab = [b"[UNK]", b"a", b"##b"]
    for wp in (mk(full - 1, 100, 2), mk(full, 100, 9), mk(full, 1025, 2), mk(0, 0, 0)):
        assert wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0, wp=wp)[0] == bad
    for wp in (mk(full, 0, 2), mk(full, 1024, 8), mk(full, 1, 0), mk(full + 8, 100, 2), False):   # (0: 100; a larger size: a newer caller; NULL: "##", 100)
        rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0, wp=wp)
        assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    rc, t = wordpiece_table(sd.dict, known, unk, nk, nu, {}, vocab, 0, wp=False)
    assert t["info"]["cont_words"] == 1 and t["info"]["max_cont_bytes"] == 1
    rc, _ = wordpiece_table(sd.dict, known, unk, nk, nu, {}, [b"a", b"##b", b"a"], 0)   # the duplicate of rule 3, both indices
    msg = L.kgpu_last_error().decode()
    assert rc == bad and " 0 " in msg and " 2 " in msg, msg
    out = C.c_void_p()
    opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), 0, 0, 0, 0)
    assert L.kgpu_vocab_create_wordpiece(None, None, None, 0, C.byref(opts), None, C.byref(out)) == bad
    assert L.kgpu_vocab_get_wordpiece_info(None, None) == bad
    from kanpyo_amd.vocab import split_words, wordpiece_opts

    with pytest.raises(ValueError):
        wordpiece_opts(b"123456789")
    with pytest.raises(ValueError):
        wordpiece_opts(b"##", 0)
    with pytest.raises(ValueError):
        wordpiece_opts(b"##", 1025)
    with pytest.raises(_lib.KgpuError):
        split_words([b"a", b"a"], [b"a"], 0)
    assert [a.tolist() for a in split_words([b"[UNK]", b"a", b"##b"], [b"ab", b"", b"ba"], 0)] == [[1, 2], [], [0]]   # opts None: "##", 100


def test_cli_argument_parsing():
    from kanpyo_amd import cli

    a = cli.parse_args(["encode", "--vocab", "v.txt"])
    assert (a.wordpiece, a.prefix, a.max_word_chars) == (False, None, None)
    a = cli.parse_args(["encode", "--vocab", "v.txt", "--wordpiece", "--prefix", "@@", "--max-word-chars", "50", "--unk", "[UNK]"])
    assert (a.wordpiece, a.prefix, a.max_word_chars, a.unk) == (True, "@@", 50, "[UNK]")
    for argv in (["encode", "--vocab", "v", "--max-word-chars", "0"], ["encode", "--vocab", "v", "--max-word-chars", "x"], ["count", "--wordpiece"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
