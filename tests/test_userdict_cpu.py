"""The user dictionary without a device (include/kanpyo_gpu.h, "user dictionary"): kgpu_userdict_host against a plain restatement of the rule
(tests/userdict_ref.py) over the naive restatement's lattices (oracle/pyref.py), against a brute-force enumeration of every path of the widened
lattice, against a dictionary that holds the entries among its own words, the crafted withdrawal cases, its protocol, the host files under the
sanitizers, and the surface of the feature -- header, binding, command line."""
import ctypes as C
import dataclasses
import os
import random
import subprocess

import numpy as np
import pytest

import mode_cases as M
import userdict_cases as U
import userdict_ref as R
from conftest import ROOT, fixture_dict_parts
from dict_cases import lattice_from_pyref
from kanpyo_amd import _lib, cli
from kanpyo_amd.mode import mode_host, mode_opts
from kanpyo_amd.nbest import connection_matrix, lattice_struct, nbest_host
from kanpyo_amd.userdict import UserDictFormatError, _entry_args, _entry_arrays, invoke_bytes, parse_csv, userdict_host

INVALID, CAPACITY = _lib.KGPU_ERR_INVALID_ARG, _lib.KGPU_ERR_CAPACITY
N_TIE_CASES = 300
N_WIDE_CASES = 300


def _check(d, s, entries, penalties=None, pd=None, get=None):
    """kgpu_userdict_host == the restatement, in all three modes -> {mode: (tokens, cost)}."""
    pd, get = pd or M.pydict_of(d), get or M.conn_get_of(d)
    lat = lattice_from_pyref(pd, s)
    conn, inv = connection_matrix(d), R.invoke_of(d, s)
    out = {}
    for m, name in enumerate(M.MODES):
        tokens, cost = userdict_host(lat, s, conn, d, entries, name, penalties)
        wt, wc = R.decode(lat, s, get, entries, inv, m, penalties or M.DEFAULTS)
        assert cost == wc and tokens.tobytes() == wt.astype(tokens.dtype).tobytes(), (s, name, penalties, entries)
        out[name] = (tokens, cost)
    return out


def _spans(tokens, classes=(1, 2, 3)) -> list:
    return [(int(t["start"]), int(t["end"])) for t in tokens if int(t["cls"]) in classes]


# ---- 1. the host function against the restatement ---------------------------------------------------------------------------------------------------------
def test_fixture_dictionary():
    from kanpyo_amd.dict import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    rng = random.Random(1)
    users = 0
    for s in M.FIXTURE_INPUTS:
        for _ in range(4):
            got = _check(d, s, U.entries_from(rng, s, 3, [-200, 0, 3000], nctx=1))
            users += any(int(t["cls"]) == 3 for t in got["normal"][0])
    assert users >= 4


def test_mode_dictionary_compounds_and_entries():
    d = M.mode_dict()
    whole = M.KANJI_COMPOUND
    # a cheap entry over the whole compound is taken in normal mode; search mode penalises it as it penalises the dictionary's own compound
    entry = [(whole, 0, 0, -100, ("user",))]
    got = _check(d, whole, entry)
    assert [int(t["cls"]) for t in got["normal"][0]] == [3, 0] and int(got["normal"][0][0]["id"]) == 1
    assert [int(t["cls"]) for t in got["search"][0]] == [1, 1, 1, 0]
    # an entry over an unknown run, beside the compound: extended mode cuts the unknown words around it and leaves the user token whole
    s = M.FILLER + whole + M.FILLER[:2]
    got = _check(d, s, [(M.FILLER, 1, 1, -500, ("user",))])
    assert _spans(got["extended"][0], (3,)) == [(0, 3)] and _spans(got["extended"][0], (2,)) == [(9, 10), (10, 11)] and _spans(got["search"][0], (2,)) == [(9, 11)]
    rng = random.Random(2)
    for s in M.compound_sentences() + M.threshold_sentences() + M.seeded_sentences(30):
        _check(d, s, U.entries_from(rng, s, rng.randint(0, 5), [0, 500, 1500], nctx=2, max_len=6))


def test_tie_dictionaries_against_the_restatement_and_brute_force():
    """The 300 seeded tie dictionaries: the restatement in three modes, and wherever EOS is reachable the minimum over EVERY path of the widened lattice
    with the path the tie rule names (lattice before user, lower (q, e) first)."""
    brute = users = ties = 0
    for seed in range(N_TIE_CASES):
        d, s, entries, pen = U.tie_user_case(seed)
        pd, get = M.pydict_of(d), M.conn_get_of(d)
        got = _check(d, s, entries, pen, pd, get)
        lat, inv = lattice_from_pyref(pd, s), R.invoke_of(d, s)
        for m, name in enumerate(M.MODES):
            want = R.brute_force(lat, s, get, entries, inv, m, pen)
            if want is None:    # EOS is not reachable: the forward's quirks decide, the restatement above has them
                continue
            brute += 1
            assert got[name][1] == want[1] and got[name][0].tobytes() == want[0].astype(got[name][0].dtype).tobytes(), (seed, name)
        users += any(int(t["cls"]) == 3 for t in got["normal"][0])
        ties += len({e[0] for e in entries}) < len(entries)
    assert brute >= N_TIE_CASES * 3 // 2 and users >= N_TIE_CASES // 5 and ties >= N_TIE_CASES // 10, (brute, users, ties)


# ---- 3. as if the entries had been in the dictionary ----------------------------------------------------------------------------------------------------------
def test_entries_behave_as_words_of_the_dictionary():
    """300 seeded dictionaries with costs from a wide range, each twice: as it is with the entries beside it, and with the entries among its own
    keywords, tokenized by oracle/pyref.py.  The cost is equal on every case; the spans (Known, Unknown and User against Known and Unknown) on every
    case whose merged lattice has a unique best path (kgpu_nbest_host with K = 2 gives two different costs).  Measured: 275 of the 300 cases are compared
    this way (0.92); the test fails below one half."""
    from oracle import pyref

    compared = 0
    for seed in range(N_WIDE_CASES):
        d, merged, s, entries = U.wide_user_case(seed)
        lat = lattice_from_pyref(M.pydict_of(d), s)
        tokens, cost = userdict_host(lat, s, connection_matrix(d), d, entries, "normal")
        pm = M.pydict_of(merged)
        mlat = lattice_from_pyref(pm, s)
        assert cost == mlat.nodes[-1].dp, (seed, s, entries)
        _, _, costs = nbest_host(mlat, connection_matrix(merged), 2)
        if len(costs) == 2 and costs[0] != costs[1]:
            compared += 1
            want = [(st, en) for _, cls, _, st, en, _ in pyref.tokenize(pm, s) if cls != 0]
            assert _spans(tokens) == want, (seed, s, entries)
    assert compared * 2 >= N_WIDE_CASES, compared


# ---- 4. withdrawal, crafted -------------------------------------------------------------------------------------------------------------------------------------
def _unknown_starts(lat, withdrawn=()) -> set:
    return {n.char_pos for i, n in enumerate(lat.nodes) if int(n.class_) == 2 and i not in withdrawn}


def test_withdrawal():
    s, entry = U.WITHDRAWAL_SENTENCE, U.WITHDRAWAL_ENTRY
    # H does not invoke: position 1 (inside the run, no known word) loses its unknown nodes and only it
    d = U.withdrawal_dict(0)
    lat = lattice_from_pyref(M.pydict_of(d), s)
    w = R.widen(lat, s, [entry], R.invoke_of(d, s))
    assert 1 in _unknown_starts(lat) and _unknown_starts(lat) - _unknown_starts(lat, w.withdrawn) == {1}
    _check(d, s, [entry])
    # an expensive entry: the path must now go AROUND the withdrawn nodes although they were cheaper
    dear = (entry[0], 1, 0, 30000, ())
    t0, c0 = userdict_host(lat, s, connection_matrix(d), d, [])
    t1, c1 = userdict_host(lat, s, connection_matrix(d), d, [dear])
    assert (1, 2) in _spans(t0, (2,)) and c1 > c0 + 20000
    assert all(st != 1 for st, _ in _spans(t1, (2,))) and (1, 3) in _spans(t1, (3,))
    _check(d, s, [dear])
    # H invokes: nothing is withdrawn
    d = U.withdrawal_dict(1)
    lat = lattice_from_pyref(M.pydict_of(d), s)
    assert R.widen(lat, s, [entry], R.invoke_of(d, s)).withdrawn == set()
    assert invoke_bytes(d, s).tolist() == [1] * len(s)
    _check(d, s, [entry])
    # a known word at the position (い at 2, and H not invoking): there was nothing to remove
    d = U.withdrawal_dict(0)
    lat = lattice_from_pyref(M.pydict_of(d), s)
    assert 2 not in _unknown_starts(lat)
    assert R.widen(lat, s, [("いう", 0, 0, 10, ())], R.invoke_of(d, s)).withdrawn == set()
    _check(d, s, [("いう", 0, 0, 10, ())])


# ---- 5. the protocol ----------------------------------------------------------------------------------------------------------------------------------------------
def _raw(ls, text: bytes, conn, rows, cols, invoke, entries, opts, tcap):
    tokens = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8)
    raw = np.frombuffer(text, dtype=np.uint8)
    arrays = entries if isinstance(entries, tuple) else _entry_arrays(entries)
    T, cost = C.c_uint64(77), C.c_int32(77)
    rc = _lib.lib().kgpu_userdict_host(C.byref(ls), raw.ctypes.data if raw.size else None, raw.size, conn.ctypes.data, rows, cols, invoke.ctypes.data if invoke is not None else None,
                                       *_entry_args(arrays), None if opts is None else C.byref(opts), tokens.ctypes.data, tcap, C.byref(T), C.byref(cost))
    return rc, tokens, T.value, cost.value


def test_capacity_one_short_and_no_entries():
    d = M.mode_dict()
    s = M.compound_sentences()[3]
    lat = lattice_from_pyref(M.pydict_of(d), s)
    conn, rows, cols = connection_matrix(d)
    ls, keep = lattice_struct(lat)
    inv = invoke_bytes(d, s)
    entries = [(M.FILLER[:2], 0, 1, -300, ()), (M.KANJI_PARTS[0], 1, 1, 10, ())]
    for name in M.MODES:
        want, cost = userdict_host(lat, s, (conn, rows, cols), d, entries, name)
        T = len(want)
        assert any(int(t["cls"]) == 3 for t in want)
        for tcap in (T - 1, 0):
            rc, tokens, t, _ = _raw(ls, s.encode(), conn, rows, cols, inv, entries, mode_opts(name), tcap)
            assert rc == CAPACITY and t == T and (tokens == 0x5A).all()
        rc, tokens, t, c = _raw(ls, s.encode(), conn, rows, cols, inv, entries, mode_opts(name), T)
        assert rc == _lib.KGPU_OK and (t, c) == (T, cost) and tokens[: T * 24].tobytes() == want.tobytes() and (tokens[T * 24 :] == 0x5A).all()
        # E = 0 is kgpu_mode_host
        mt, mc = mode_host(lat, s, (conn, rows, cols), name)
        ut, uc = userdict_host(lat, s, (conn, rows, cols), d, [], name)
        assert (mc, mt.tobytes()) == (uc, ut.tobytes())
    rc, tokens, t, c = _raw(ls, s.encode(), conn, rows, cols, None, [], None, 100)     # no invoke bytes, no options: normal mode
    assert rc == _lib.KGPU_OK and tokens[: t * 24].tobytes() == mode_host(lat, s, (conn, rows, cols), "normal")[0].tobytes()
    del keep


def test_every_refused_argument():
    d = M.mode_dict()
    s = M.THRESHOLD[1][0] + M.FILLER
    lat = lattice_from_pyref(M.pydict_of(d), s)
    conn, rows, cols = connection_matrix(d)
    inv = invoke_bytes(d, s)
    good = [("大阪", 0, 1, 5, ())]

    def rc_of(entries=good, change=lambda ls, keep: None, opts=None, text=s.encode(), rows=rows, cols=cols, invoke=inv):
        ls, keep = lattice_struct(lat)
        change(ls, keep)
        return _raw(ls, text, conn, rows, cols, invoke, entries, opts or mode_opts("search"), 1000)[0]

    def raw_entry(key: bytes, left=0, right=0):
        return (np.frombuffer(key, dtype=np.uint8), np.array([0, len(key)], dtype=np.uint64), np.array([left], dtype=np.uint16), np.array([right], dtype=np.uint16),
                np.array([0], dtype=np.int16))

    assert rc_of() == _lib.KGPU_OK
    empty = (np.frombuffer(b"a", dtype=np.uint8), np.array([0, 1, 1], dtype=np.uint64), np.zeros(2, np.uint16), np.zeros(2, np.uint16), np.zeros(2, np.int16))
    assert rc_of(empty) == INVALID and b"empty" in _lib.lib().kgpu_last_error()
    assert rc_of(raw_entry(("あ" * 65).encode())) == INVALID and rc_of(raw_entry(("あ" * 64).encode())) == _lib.KGPU_OK       # 64 characters, 192 bytes
    assert rc_of(raw_entry(b"x" * 64)) == _lib.KGPU_OK and rc_of(raw_entry(b"x" * 65)) == INVALID
    assert rc_of(raw_entry(("𠀀" * 63 + "あ").encode())) == _lib.KGPU_OK and rc_of(raw_entry(("𠀀" * 64).encode())) == INVALID   # 255 and 256 bytes
    for notutf8 in (b"\xff", b"\xe3\x81", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"a\x80"):
        assert rc_of(raw_entry(notutf8)) == INVALID, notutf8
    assert rc_of(raw_entry(b"a", left=cols)) == INVALID and rc_of(raw_entry(b"a", right=rows)) == INVALID and rc_of(raw_entry(b"a", cols - 1, rows - 1)) == _lib.KGPU_OK
    two = (np.frombuffer(b"ab", dtype=np.uint8), np.array([0, 2, 1], dtype=np.uint64), np.zeros(2, np.uint16), np.zeros(2, np.uint16), np.zeros(2, np.int16))
    assert rc_of(two) == INVALID                                                          # offsets that run backwards
    assert rc_of(invoke=None) == INVALID                                                  # entries and characters, but no invoke bytes
    assert rc_of(opts=_lib.ModeOpts(3, 2, 3000, 7, 1700)) == INVALID
    # kgpu_mode_host's checks of the lattice and the text
    assert rc_of(change=lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes))) == INVALID
    assert rc_of(change=lambda ls, keep: setattr(keep[0][2], "left_id", 2)) == INVALID
    assert rc_of(change=lambda ls, keep: setattr(keep[0][1], "end_char", len(s) + 1)) == INVALID
    assert rc_of(change=lambda ls, keep: setattr(ls, "n_nodes", 1)) == INVALID
    assert rc_of(change=lambda ls, keep: setattr(ls, "n_positions", len(s) + 1)) == INVALID and b"positions" in _lib.lib().kgpu_last_error()   # fewer than C + 2
    assert rc_of([], change=lambda ls, keep: setattr(ls, "n_positions", len(s) + 1), invoke=None) == INVALID
    # two neighbours with their places swapped, every other field and every edge still right: the nodes are no longer numbered by start position
    t = next(t for t in range(1, len(lat.nodes) - 2) if lat.nodes[t].char_pos < lat.nodes[t + 1].char_pos and lat.nodes[t].end_char != lat.nodes[t + 1].char_pos)
    swap = {t: t + 1, t + 1: t}
    nodes = list(lat.nodes)
    nodes[t], nodes[t + 1] = nodes[t + 1], nodes[t]
    swapped = dataclasses.replace(lat, nodes=nodes, edges=[sorted(swap.get(j, j) for j in e) for e in lat.edges])
    ls, keep = lattice_struct(swapped)
    assert _raw(ls, s.encode(), conn, rows, cols, inv, good, mode_opts("search"), 1000)[0] == INVALID
    assert b"not numbered by start position" in _lib.lib().kgpu_last_error() and f"node {t + 1}:".encode() in _lib.lib().kgpu_last_error()
    assert rc_of(text=s.encode()[:-1]) == INVALID and rc_of(text=b"\xff" + s.encode()[1:]) == INVALID
    with pytest.raises(ValueError):
        _entry_arrays([("a", 70000, 0, 0)])


def test_csv():
    text = '# a comment\n\nGPU,1,2,-50,名詞,固有名詞\n"a,b",0,0,10,"x,y",z\nＧＰＵ,3,4,5\n'
    got = parse_csv(text)
    assert [tuple(e) for e in got] == [("GPU", 1, 2, -50, ("名詞", "固有名詞")), ("a,b", 0, 0, 10, ("x,y", "z")), ("ＧＰＵ", 3, 4, 5, ())]
    assert parse_csv(text, "NFKC")[2].surface == "GPU"           # a full-width key through the normaliser
    assert parse_csv("ｶﾞ,0,0,0\n", "NFKC")[0].surface == "ガ" and parse_csv("ｶﾞ,0,0,0\n")[0].surface == "ｶﾞ"
    # '\n' alone ends a line (a '\r' in front of it goes): a surface may hold the other characters str.splitlines would cut at
    assert [e.surface for e in parse_csv("a\u2028b,0,0,0\r\nc\x85d,0,0,0\ne\x0cf,1,1,1")] == ["a\u2028b", "c\x85d", "e\x0cf"]
    for bad, line in (("a,1,2\n", 1), ("ok,0,0,0\nb,x,0,0\n", 2), (",0,0,0\n", 1), ("a,0,0,40000\n", 1), ("a,0,0,0\n\nb,-1,0,0\n", 3), ('a,0,0,0\n"b,0,0,0\n', 2)):
        with pytest.raises(UserDictFormatError) as e:
            parse_csv(bad)
        assert e.value.line == line and f"line {line}" in str(e.value), bad


# ---- 6. the host files under the sanitizers --------------------------------------------------------------------------------------------------------------------
def test_host_files_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/c_abi/userdict_sanitize.cpp, its own main) linked with kgpu_user_host.cpp and kgpu_user_table.cpp alone: nothing is
    loaded into Python."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):   # (the probe of tests/test_mode_cpu.py, before any work)
        pytest.skip("no libasan in this toolchain")
    exe = str(tmp_path / "userdict_sanitize")
    csrc = os.path.join(ROOT, "kanpyo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "userdict_sanitize.cpp"), os.path.join(csrc, "kgpu_user_host.cpp"), os.path.join(csrc, "kgpu_user_table.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "userdict sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 7. the surface -----------------------------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "kanpyo_gpu.h"\nint main(void) { kgpu_userdict_info i = {0, 0, 0, 0}; kgpu_token t = {1, KGPU_CLASS_USER, 0, 0, 1, 1};\n'
                   "  return (int)i.entries + (t.cls != 3) + (KGPU_USERDICT_MAX_KEY_CHARS != 64) + (KGPU_USERDICT_MAX_KEY_BYTES != 255)\n"
                   "         + (sizeof(&kgpu_userdict_create) + sizeof(&kgpu_userdict_host) + sizeof(&kgpu_tokenize_batch_user) + sizeof(&kgpu_userdict_destroy) == 0); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_new_symbols_header_and_makefile():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "kanpyo_gpu.h"), encoding="utf-8").read()
    for s, nargs in (("kgpu_userdict_create", 8), ("kgpu_userdict_destroy", 1), ("kgpu_userdict_get_info", 2), ("kgpu_userdict_host", 18), ("kgpu_tokenize_batch_user", 12)):
        assert s in _lib.SYMBOLS and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs and s + "(" in header, s
    assert "user dictionary" in header and "#define KGPU_CLASS_USER 3" in header and "8 N + 32 U + 16 C + 44" in header and C.sizeof(_lib.UserdictInfo) == 32
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_user.hip") == 2 and all(f in mk for f in ("kgpu_user_host.cpp", "kgpu_user_batch.cpp", "kgpu_user_table.cpp", "kgpu_user_core.h"))
    import kanpyo_amd
    from kanpyo_amd.tokenizer import Tokenizer

    assert kanpyo_amd.userdict_host is userdict_host and {"UserDict", "UserEntry", "userdict_host"} <= set(kanpyo_amd.__all__)
    assert kanpyo_amd.TokenClass.USER == 3 and kanpyo_amd.TokenClass(3) is kanpyo_amd.TokenClass.User
    assert callable(Tokenizer.tokenize_user) and callable(Tokenizer.tokenize_user_packed) and callable(kanpyo_amd.UserDict.from_csv)
    # the table's hash is the other byte-keyed tables' (tests/table_keys.py builds its worst cases with that one)
    import encode_ref

    for key in (b"a", b"abcdefg", "関西".encode()):
        assert L.kgpu_debug_userdict_hash(key, len(key)) == encode_ref.key_hash(key)
    assert L.kgpu_debug_userdict_slots(34) == 128 and L.kgpu_debug_userdict_slots(0) == 16
    worst = U.table_worst_keys()
    col = [k.encode() for k in worst["colliding"]]
    assert all(encode_ref.key_hash(col[i]) == encode_ref.key_hash(col[i + 1]) and col[i] != col[i + 1] for i in range(0, len(col), 2))
    assert len({encode_ref.key_hash(k.encode()) & 63 for k in worst["crowded"]}) == 1


def test_cli_parses_user_dict_and_refuses_what_does_not_go_with_it(tmp_path, capsys):
    good = tmp_path / "user.csv"
    good.write_text("GPU,1,1,-50,名詞,固有名詞\nｶﾞ,0,0,10,x\n", encoding="utf-8")
    a = cli.parse_args(["tokenize", "-c", "x.dict", "--user-dict", str(good)])
    assert (a.command, a.mode, a.split) == ("tokenize", None, "host") and [e.surface for e in a.user_entries] == ["GPU", "ｶﾞ"]
    a = cli.parse_args(["tokenize", "--user-dict", str(good), "--mode", "search", "--mode-penalties", "3,100,5,200", "--normalize", "nfkc", "--sentences"])
    assert (a.mode, a.mode_penalties, a.normalize, a.sentences) == ("search", (3, 100, 5, 200), "nfkc", True) and [e.surface for e in a.user_entries] == ["GPU", "ガ"]
    assert cli.parse_args(["tokenize"]).user_entries is None and getattr(cli.parse_args([]), "user_entries", None) is None
    bad = tmp_path / "bad.csv"
    bad.write_text("GPU,1,1,-50\nbroken,1\n", encoding="utf-8")
    capsys.readouterr()
    for argv in (["--user-dict", str(good), "--split", "device"], ["--user-dict", str(good), "--nbest", "2"], ["--user-dict", str(good), "--marginal"],
                 ["--user-dict", str(good), "--sample", "3"], ["--user-dict", str(tmp_path / "none.csv")], ["--user-dict", str(bad)]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["tokenize"] + argv)
        out = capsys.readouterr()
        assert e.value.code == 2 and out.out == "", argv
    assert "line 2" in out.err
    with pytest.raises(SystemExit):
        cli.parse_args(["wakati", "--user-dict", str(good)])   # tokenize's option alone
