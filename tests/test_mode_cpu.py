"""Search and extended modes without a device (include/kanpyo_gpu.h, "search mode"): kgpu_mode_host against a plain restatement of the rule
(tests/mode_ref.py) over the naive restatement's lattices (oracle/pyref.py), against tokenize's own backtrace where every penalty is 0, against a
brute-force enumeration of every path, its protocol, the host file under the sanitizers, and the surface of the feature -- header, binding, command
line."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import mode_cases as M
import mode_ref as R
from conftest import ROOT, fixture_dict_parts
from dict_cases import lattice_from_pyref
from kanpyo_amd import _lib, cli
from kanpyo_amd.mode import mode_host, mode_opts
from kanpyo_amd.nbest import connection_matrix, lattice_struct

INVALID, CAPACITY = _lib.KGPU_ERR_INVALID_ARG, _lib.KGPU_ERR_CAPACITY
N_TIE_CASES = 300
N_SEEDED = 120


def _check(d, sentences, penalties=None, pd=None, get=None):
    """kgpu_mode_host == the restatement, in all three modes -> {(sentence, mode): (tokens, cost)}."""
    pd, get = pd or M.pydict_of(d), get or M.conn_get_of(d)
    conn = connection_matrix(d)
    out = {}
    for s in sentences:
        lat = lattice_from_pyref(pd, s)
        for m, name in enumerate(M.MODES):
            tokens, cost = mode_host(lat, s, conn, name, penalties)
            wt, wc = R.decode(lat, s, get, m, penalties or M.DEFAULTS)
            assert cost == wc and tokens.tobytes() == wt.astype(tokens.dtype).tobytes(), (s, name, penalties)
            out[s, name] = (tokens, cost)
    return out


def _surfaces(s: str, tokens) -> list:
    raw = s.encode("utf-8")
    return [raw[int(t["position"]) : int(t["position"]) + int(t["byte_len"])].decode("utf-8") for t in tokens if int(t["cls"]) != 0]


# ---- 1. the host function against the restatement ---------------------------------------------------------------------------------------------------------
def test_fixture_dictionary():
    from kanpyo_amd.dict import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    got = _check(d, M.FIXTURE_INPUTS)
    assert any(len(t) == 0 for (_, m), (t, _) in got.items() if m == "normal")          # an unreachable EOS among them: no records
    assert len(got["", "search"][0]) == 1 and got["", "search"][1] == M.conn_get_of(d)(0, 0)   # "": [EOS], cost M[0][0]


def test_compounds_give_way_to_their_parts():
    d = M.mode_dict()
    got = _check(d, M.compound_sentences())
    for whole, parts in ((M.KANJI_COMPOUND, M.KANJI_PARTS), (M.KANA_COMPOUND, M.KANA_PARTS)):
        assert _surfaces(whole, got[whole, "normal"][0]) == [whole]
        assert _surfaces(whole, got[whole, "search"][0]) == list(parts) == _surfaces(whole, got[whole, "extended"][0])
    s = M.compound_sentences()[3]   # unknown words between the compounds: extended mode cuts them into characters, search mode does not
    assert _surfaces(s, got[s, "search"][0]) == [M.FILLER] + list(M.KANJI_PARTS) + [M.FILLER[:2]] + list(M.KANA_PARTS) + [M.FILLER[:1]]
    assert _surfaces(s, got[s, "extended"][0]) == list(M.FILLER) + list(M.KANJI_PARTS) + list(M.FILLER[:2]) + list(M.KANA_PARTS) + [M.FILLER[:1]]
    assert got[s, "search"][1] == got[s, "extended"][1]


def test_length_thresholds():
    d = M.mode_dict()
    got = _check(d, M.threshold_sentences())
    for whole, parts, split in M.THRESHOLD:
        assert _surfaces(whole, got[whole, "normal"][0]) == [whole]
        assert _surfaces(whole, got[whole, "search"][0]) == M.surfaces_of(whole, parts, split), whole
    # other lengths move the thresholds: nothing is long at 9 / 9; at 3 / 8 each rule begins one character later
    for pen, splits in (((9, 3000, 9, 1700), [False] * 8), ((3, 3000, 8, 1700), [False, False, True, False, False, True, False, True])):
        got = _check(d, [w for w, _, _ in M.THRESHOLD], pen)
        for (whole, parts, _), split in zip(M.THRESHOLD, splits):
            assert _surfaces(whole, got[whole, "search"][0]) == M.surfaces_of(whole, parts, split), (whole, pen)


def test_every_edge_of_the_kanji_list():
    d = M.mode_dict()
    got = _check(d, M.edge_sentences())
    kanji = []
    for cp in M.EDGE_CHARS:
        s = M.edge_word(cp)
        assert _surfaces(s, got[s, "normal"][0]) == [s]
        assert _surfaces(s, got[s, "search"][0]) == (["山", chr(cp) + "川"] if M.is_kanji_case(cp) else [s]), hex(cp)
        kanji.append(M.is_kanji_case(cp))
    assert sum(kanji) == 10 and len(kanji) == 20   # each range from both sides


def test_crowded_positions_and_long_nodes():
    _check(M.crowded_dict(), [M.CROWDED_SENTENCE, M.CROWDED_SENTENCE[::-1]])
    d = M.wide_dict()
    assert max(len(e) for e in lattice_from_pyref(M.pydict_of(d), M.CROWDED_SENTENCE).edges) > 64
    for pen in (None, (1, 100, 1, 100), (2, 0, 2, 100)):
        _check(d, [M.CROWDED_SENTENCE, M.CROWDED_SENTENCE[::-1]], pen)
    d = M.long_dict()
    got = _check(d, M.LONG_SENTENCES)
    s65, s1025 = M.LONG_SENTENCES[:2]
    assert len(got[s65, "search"][0]) == 2 and len(got[s65, "extended"][0]) == 66
    assert [int(t["end"]) - int(t["start"]) for t in got[s1025, "search"][0]] == [1024, 1, 3]   # the reference's cap on an unknown word, then the rest, then EOS
    assert len(got[s1025, "extended"][0]) == 1026 and got[s1025, "search"][1] == got[s1025, "normal"][1] + 1022 * 3000


def test_tie_dictionaries_against_the_restatement_and_brute_force():
    differ = brute = 0
    for seed in range(N_TIE_CASES):
        d, s, pen = M.tie_mode_case(seed)
        pd, get = M.pydict_of(d), M.conn_get_of(d)
        got = _check(d, [s], pen, pd, get)
        lat = lattice_from_pyref(pd, s)
        for m, name in enumerate(M.MODES):
            want = R.brute_force(lat, s, get, m, pen)
            if want is None:    # EOS is not reachable: the forward's quirks decide, the restatement above has them
                continue
            brute += 1
            assert got[s, name][1] == want[1] and got[s, name][0].tobytes() == want[0].tobytes(), (seed, name)
        differ += got[s, "search"][0].tobytes() != got[s, "normal"][0].tobytes()
    assert brute >= N_TIE_CASES * 3 // 2 and differ >= N_TIE_CASES // 20, (brute, differ)


# ---- 2. without penalties it is tokenize ------------------------------------------------------------------------------------------------------------------
def test_no_penalty_is_the_lattices_own_backtrace():
    """NORMAL, and SEARCH with both penalties 0, give the records of the lattice's own dp / pre -- tokenize's backtrace -- on every sentence, the ones
    whose EOS is unreachable included."""
    from kanpyo_amd.dict import Dict
    from nbest_ref import records_of

    cases = [(Dict.from_parts(**fixture_dict_parts()), M.FIXTURE_INPUTS), (M.mode_dict(), M.compound_sentences() + M.threshold_sentences() + M.seeded_sentences(20))]
    cases += [(M.tie_mode_case(seed)[0], [M.tie_mode_case(seed)[1]]) for seed in range(60)]
    empty = 0
    for d, sents in cases:
        pd, conn = M.pydict_of(d), connection_matrix(d)
        for s in sents:
            lat = lattice_from_pyref(pd, s)
            want = records_of(lat, R.chain([n.pre for n in lat.nodes]))
            for mode, pen in (("normal", (0, 99999, 0, 99999)), ("search", (2, 0, 7, 0)), ("extended", (1, 0, 1, 0))):
                tokens, cost = mode_host(lat, s, conn, mode, pen)
                if mode != "extended":
                    assert tokens.tobytes() == want.astype(tokens.dtype).tobytes(), (s, mode)
                assert cost == lat.nodes[-1].dp, (s, mode)
            empty += len(want) == 0
    assert empty >= 2


# ---- 3. the sweep is not vacuous --------------------------------------------------------------------------------------------------------------------------
def test_seeded_sentences_differ_between_the_modes():
    d = M.mode_dict()
    sents = M.seeded_sentences(N_SEEDED)
    got = _check(d, sorted(set(sents)))
    search = sum(got[s, "search"][0].tobytes() != got[s, "normal"][0].tobytes() for s in sents)
    extended = sum(got[s, "extended"][0].tobytes() != got[s, "search"][0].tobytes() for s in sents)
    assert search * 3 >= N_SEEDED and extended * 10 >= N_SEEDED, (search, extended)


# ---- 4. the protocol --------------------------------------------------------------------------------------------------------------------------------------
def _raw(ls, text: bytes, conn, rows, cols, opts, tcap, null_opts=False):
    tokens = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8)
    raw = np.frombuffer(text, dtype=np.uint8)
    T, cost = C.c_uint64(77), C.c_int32(77)
    rc = _lib.lib().kgpu_mode_host(C.byref(ls), raw.ctypes.data if raw.size else None, raw.size, conn.ctypes.data, rows, cols, None if null_opts else C.byref(opts),
                                   tokens.ctypes.data, tcap, C.byref(T), C.byref(cost))
    return rc, tokens, T.value, cost.value


def test_capacity_one_short():
    d = M.mode_dict()
    s = M.compound_sentences()[3]
    lat = lattice_from_pyref(M.pydict_of(d), s)
    conn, rows, cols = connection_matrix(d)
    ls, keep = lattice_struct(lat)
    for name in M.MODES:
        want, cost = mode_host(lat, s, d, name)
        T = len(want)
        for tcap in (T - 1, 0):
            rc, tokens, t, _ = _raw(ls, s.encode(), conn, rows, cols, mode_opts(name), tcap)
            assert rc == CAPACITY and t == T and (tokens == 0x5A).all()
        rc, tokens, t, c = _raw(ls, s.encode(), conn, rows, cols, mode_opts(name), T)
        assert rc == _lib.KGPU_OK and (t, c) == (T, cost) and tokens[: T * 24].tobytes() == want.tobytes() and (tokens[T * 24 :] == 0x5A).all()
    del keep


def test_invalid_options_and_contradictory_lattices():
    d = M.mode_dict()
    s = M.THRESHOLD[1][0] + M.FILLER
    lat = lattice_from_pyref(M.pydict_of(d), s)
    conn, rows, cols = connection_matrix(d)

    def rc_of(change=lambda ls, keep: None, opts=None, text=s.encode(), rows=rows, cols=cols, null_opts=False):
        ls, keep = lattice_struct(lat)
        change(ls, keep)
        return _raw(ls, text, conn, rows, cols, opts or mode_opts("search"), 1000, null_opts)[0]

    assert rc_of() == _lib.KGPU_OK
    assert rc_of(opts=_lib.ModeOpts(3, 2, 3000, 7, 1700)) == INVALID and b"mode" in _lib.lib().kgpu_last_error()
    for k in range(3):
        o = mode_opts("extended")
        o.reserved[k] = 1
        assert rc_of(opts=o) == INVALID
    assert rc_of(null_opts=True) == INVALID
    assert rc_of(opts=_lib.ModeOpts(0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == _lib.KGPU_OK        # any numbers are options
    assert rc_of(lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes))) == INVALID            # an edge node out of range
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "end_char", 0) or setattr(keep[0][1], "char_pos", 1)) == INVALID   # end_char < char_pos
    assert rc_of(lambda ls, keep: setattr(keep[0][2], "left_id", 2)) == INVALID                 # a context id outside the matrix
    assert rc_of(cols=1) == INVALID
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "char_pos", 99)) == INVALID               # starts behind the last position
    assert rc_of(lambda ls, keep: setattr(ls, "n_nodes", 1)) == INVALID
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "byte_len", len(s.encode()) + 1)) == INVALID   # bytes beyond the text
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "end_char", len(s) + 1)) == INVALID       # ends behind the text's characters
    assert rc_of(text=s.encode()[:-1]) == INVALID                                               # text cut inside a character
    assert rc_of(text=b"\xff" + s.encode()[1:]) == INVALID
    with pytest.raises(ValueError):
        mode_opts("fast")
    with pytest.raises(ValueError):
        mode_opts("search", (1, 2, 3))


# ---- 5. the host file under the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_host_function_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/c_abi/mode_sanitize.cpp, its own main) linked with kgpu_mode_host.cpp alone: nothing is loaded into Python."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):   # (the probe of tests/test_prob_cpu.py, before any work)
        pytest.skip("no libasan in this toolchain")
    exe = str(tmp_path / "mode_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "mode_sanitize.cpp"), os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_mode_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mode sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---- 6. the surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_header_and_makefile():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "kanpyo_gpu.h"), encoding="utf-8").read()
    for s, nargs in (("kgpu_mode_host", 11), ("kgpu_tokenize_batch_mode", 11)):
        assert s in _lib.SYMBOLS and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs and s + "(" in header, s
    assert "search mode" in header and "#define KGPU_MODE_EXTENDED 2u" in header and C.sizeof(_lib.ModeOpts) == 32
    assert (_lib.KGPU_MODE_NORMAL, _lib.KGPU_MODE_SEARCH, _lib.KGPU_MODE_EXTENDED) == (0, 1, 2)
    o = mode_opts()
    assert (o.mode, o.kanji_length, o.kanji_penalty, o.other_length, o.other_penalty, list(o.reserved)) == (1, 2, 3000, 7, 1700, [0, 0, 0])
    assert "{(m), 2u, 3000u, 7u, 1700u, {0u, 0u, 0u}}" in header
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_mode.hip") == 2 and "kgpu_mode_host.cpp" in mk and "kgpu_mode_batch.cpp" in mk and "kgpu_mode_core.h" in mk
    import kanpyo_amd
    from kanpyo_amd.tokenizer import Tokenizer

    assert kanpyo_amd.mode_host is mode_host and "mode_host" in kanpyo_amd.__all__
    assert callable(Tokenizer.tokenize_mode) and callable(Tokenizer.tokenize_mode_packed)


def test_cli_parses_mode_and_refuses_what_does_not_go_with_it(capsys):
    a = cli.parse_args(["tokenize", "-c", "x.dict", "--mode", "search"])
    assert (a.command, a.mode, a.mode_penalties, a.split, a.normalize) == ("tokenize", "search", None, "host", "none")
    a = cli.parse_args(["tokenize", "関西国際空港", "--mode", "extended", "--mode-penalties", "3,100,5,200", "--normalize", "nfkc"])
    assert (a.input, a.mode, a.mode_penalties, a.normalize) == ("関西国際空港", "extended", (3, 100, 5, 200), "nfkc")
    assert cli.parse_args(["tokenize", "--mode", "normal"]).mode == "normal"
    assert cli.parse_args(["tokenize"]).mode is None and cli.parse_args([]).mode is None
    for bad in (["--mode", "fast"], ["--mode", "search", "--split", "device"], ["--mode", "search", "--nbest", "2"], ["--mode", "search", "--marginal"],
                ["--mode", "extended", "--sample", "3"], ["--mode-penalties", "1,2,3,4"], ["--mode", "search", "--mode-penalties", "1,2,3"],
                ["--mode", "search", "--mode-penalties", "1,2,3,x"], ["--mode", "search", "--mode-penalties", "1,2,3,4294967296"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["tokenize"] + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_args(["wakati", "--mode", "search"])   # tokenize's option alone
