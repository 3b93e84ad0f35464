"""Search and extended modes on the device (include/kanpyo_gpu.h, "search mode"): kgpu_tokenize_batch_mode, Tokenizer.tokenize_mode* and
`python -m kanpyo_amd tokenize --mode`.  The device must equal kgpu_mode_host applied to kgpu_lattice_dump of the same sentence, byte for byte:
records, tok_offsets, costs and status.  The host function itself is pinned to a plain restatement and to brute force in tests/test_mode_cpu.py; the dump is
compared with the naive restatement's lattice node for node, and this call with the host rule over the restatement's lattices, in
tests/test_gpu_lattice_sweep.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mode_cases as M
from conftest import ROOT, fixture_dict_parts

pytestmark = pytest.mark.gpu

INF, NO_SCRATCH = 1 << 30, 2


def _tok(d):
    from kanpyo_amd import Tokenizer, _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return Tokenizer(d)


def _want(tok, d, sents, mode, penalties=None):
    """kgpu_mode_host over kgpu_lattice_dump, sentence after sentence (each distinct one once) -> the arrays of the batch call (a sentence given as
    bytes is not UTF-8: no records, cost 1 << 30, status 1)."""
    from kanpyo_amd.lattice import dump_lattice
    from kanpyo_amd.mode import mode_host
    from kanpyo_amd.nbest import connection_matrix
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    conn = connection_matrix(d)
    tokens, toff, costs, status, seen = [], [0], [], [], {}
    for s in sents:
        if isinstance(s, bytes):
            toff.append(toff[-1])
            costs.append(INF)
            status.append(1)
            continue
        if s not in seen:
            seen[s] = mode_host(dump_lattice(tok, s), s, conn, mode, penalties)
        t, c = seen[s]
        tokens.append(t)
        toff.append(toff[-1] + len(t))
        costs.append(c)
        status.append(0)
    return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(toff, dtype=np.uint64), np.array(costs, dtype=np.int32),
            np.array(status, dtype=np.uint8))


def _got(tok, sents, mode, penalties=None):
    from kanpyo_amd.tokenizer import pack_sentences

    return tok.tokenize_mode_packed(*pack_sentences(sents), mode, penalties)


def _equal(got, want, what=""):
    for name, g, w in zip(("tokens", "tok_offsets", "costs", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def _surfaces(s: str, tokens) -> list:
    raw = s.encode("utf-8")
    return [raw[int(t["position"]) : int(t["position"]) + int(t["byte_len"])].decode("utf-8") for t in tokens if int(t["cls"]) != 0]


@pytest.fixture(scope="module")
def fixture_tok():
    from kanpyo_amd import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    return d, _tok(d)


@pytest.fixture(scope="module")
def mode_tok():
    d = M.mode_dict()
    return d, _tok(d)


@pytest.fixture(scope="module")
def synth_tok():
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=11)
    return sd, _tok(sd.dict)


@pytest.mark.parametrize("mode", M.MODES)
def test_fixture_sentences(fixture_tok, mode):
    d, tok = fixture_tok
    got = _got(tok, M.FIXTURE_INPUTS, mode)
    _equal(got, _want(tok, d, M.FIXTURE_INPUTS, mode))
    counts = np.diff(got[1].astype(np.int64)).tolist()
    assert counts[0] == 1 and 0 in counts and not got[3].any()   # "": [EOS]; an EOS without a predecessor: no records, status 0
    if mode == "normal":
        from kanpyo_amd.tokenizer import pack_sentences

        plain = tok.tokenize_packed(*pack_sentences(M.FIXTURE_INPUTS))
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tolist() == plain[1].tolist()   # the quirks of an unreachable EOS included


@pytest.mark.parametrize("mode", M.MODES)
def test_compounds_thresholds_and_edges(mode_tok, mode):
    d, tok = mode_tok
    sents = M.compound_sentences() + M.threshold_sentences() + M.edge_sentences()
    got = _got(tok, sents, mode)
    _equal(got, _want(tok, d, sents, mode))
    off = got[1].tolist()
    rows = {s: _surfaces(s, got[0][off[i] : off[i + 1]]) for i, s in enumerate(sents)}
    split = mode != "normal"
    assert rows[M.KANJI_COMPOUND] == M.surfaces_of(M.KANJI_COMPOUND, M.KANJI_PARTS, split) and rows[M.KANA_COMPOUND] == M.surfaces_of(M.KANA_COMPOUND, M.KANA_PARTS, split)
    for whole, parts, searched in M.THRESHOLD:
        assert rows[whole] == M.surfaces_of(whole, parts, split and searched), whole
    for cp in M.EDGE_CHARS:
        assert rows[M.edge_word(cp)] == M.surfaces_of(M.edge_word(cp), ("山", chr(cp) + "川"), split and M.is_kanji_case(cp)), hex(cp)
    filler = rows[M.compound_sentences()[3]][:3]
    assert filler == (list(M.FILLER) if mode == "extended" else [M.FILLER] + list(M.KANJI_PARTS[:2]) if split else [M.FILLER, M.KANJI_COMPOUND, M.FILLER[:2]])
    # other penalties than the defaults
    for pen in ((3, 3000, 8, 1700), (0, 1, 0, 1), (2, 0xFFFFFFFF, 7, 0xFFFFFFFF)):
        _equal(_got(tok, sents, mode, pen), _want(tok, d, sents, mode, pen), pen)


@pytest.mark.parametrize("mode", M.MODES)
def test_crowded_positions(mode):
    """The crowded dictionary of the N-best tests, and a wide one whose targets have more than 64 predecessors: more than one round of the forward
    kernel's lanes."""
    from kanpyo_amd.lattice import dump_lattice

    sents = [M.CROWDED_SENTENCE, M.CROWDED_SENTENCE[::-1], "あ" * 9]
    for d, widest in ((M.crowded_dict(), 8), (M.wide_dict(), 64)):
        tok = _tok(d)
        assert max(len(e) for e in dump_lattice(tok, sents[0]).edges) > widest
        for pen in (None, (1, 100, 1, 100), (2, 0, 2, 100)):
            _equal(_got(tok, sents, mode, pen), _want(tok, d, sents, mode, pen), pen)
        tok.close()


@pytest.mark.parametrize("mode", M.MODES)
def test_long_nodes(mode):
    """Unknown words of 65 and of 1024 characters: a node longer than a wavefront, the reference's cap, an extended split longer than 64."""
    d = M.long_dict()
    tok = _tok(d)
    got = _got(tok, M.LONG_SENTENCES, mode)
    _equal(got, _want(tok, d, M.LONG_SENTENCES, mode))
    assert np.diff(got[1].astype(np.int64)).tolist() == ([66, 1026, 68] if mode == "extended" else [2, 3, 4])
    tok.close()


def test_tie_dictionaries():
    rng = random.Random(77)
    for seed in range(8):   # 8 dictionaries x 25 sentences, each in the three modes
        d = M.tie_dict(2000 + seed)
        tok = _tok(d)
        sents = [M.tie_sentence(rng) for _ in range(25)]
        pen = M.tie_penalties(rng)
        for mode in M.MODES:
            _equal(_got(tok, sents, mode, pen), _want(tok, d, sents, mode, pen), (seed, mode, pen))
        tok.close()


def test_invalid_utf8_and_an_empty_sentence_in_the_middle(mode_tok):
    d, tok = mode_tok
    sents = [M.KANJI_COMPOUND, b"\xe3\x81", "", M.KANA_COMPOUND, b"\xff", M.FILLER]
    for mode in M.MODES:
        got = _got(tok, sents, mode)
        _equal(got, _want(tok, d, sents, mode))
        assert got[3].tolist() == [0, 1, 0, 0, 1, 0] and got[1][1] == got[1][2] and got[1][3] - got[1][2] == 1 and got[2][1] == INF


def test_1025_sentences_cross_the_chunk(mode_tok, monkeypatch):
    d, tok = mode_tok
    words = [M.KANJI_COMPOUND, M.KANA_COMPOUND, "東京", "大阪府", M.FILLER, "空港"]
    sents = [words[(i * 7 + i // 5) % len(words)] for i in range(1025)]
    monkeypatch.delenv("KGPU_HOST_MODE_CHUNK_SENTS", raising=False)
    for mode in ("search", "extended"):
        one = _got(tok, sents, mode)
        _equal(one, _want(tok, d, sents, mode))
        monkeypatch.setenv("KGPU_HOST_MODE_CHUNK_SENTS", "3")
        _equal(_got(tok, sents, mode), one, mode)
        monkeypatch.delenv("KGPU_HOST_MODE_CHUNK_SENTS")


def test_arena_protocol(fixture_tok, monkeypatch):
    """The kept lattices and their slabs outgrow the arena: the chunk runs again on a doubled one (KGPU_HOST_MODE_ARENA_INITIAL bounds the first); at
    the largest arena (KGPU_HOST_MODE_ARENA_MAX) the chunk is halved until the sentence that alone does not fit is left with KGPU_SENT_NO_SCRATCH and
    no records, its neighbours' records being what they always are."""
    d, tok = fixture_tok
    long_ = "辞書形態素あ" * 25
    sents = M.FIXTURE_INPUTS + [long_] + M.FIXTURE_INPUTS[::-1]
    want = _got(tok, sents, "search")
    _equal(want, _want(tok, d, sents, "search"))
    monkeypatch.setenv("KGPU_HOST_MODE_ARENA_INITIAL", "2048")
    tok.routing(reset=True)
    _equal(_got(tok, sents, "search"), want)   # regrows until everything fits
    assert tok.routing()["arena_regrows"] >= 3
    monkeypatch.setenv("KGPU_HOST_MODE_ARENA_MAX", "8192")
    got = _got(tok, sents, "search")
    assert got[3].tolist() == [0] * 6 + [NO_SCRATCH] + [0] * 6 and got[2][6] == INF
    short = [s for s in sents if s != long_]
    monkeypatch.delenv("KGPU_HOST_MODE_ARENA_INITIAL")
    monkeypatch.delenv("KGPU_HOST_MODE_ARENA_MAX")
    rest = _got(tok, short, "search")
    assert got[1][6] == got[1][7] and got[0].tobytes() == rest[0].tobytes()
    assert np.delete(got[1], 7).tolist() == rest[1].tolist() and np.delete(got[2], 6).tolist() == rest[2].tolist()
    _equal(_got(tok, sents, "search"), want)


def test_capacity_one_short(mode_tok):
    from kanpyo_amd import _lib
    from kanpyo_amd.mode import mode_opts
    from kanpyo_amd.tokenizer import TOKEN_DTYPE, pack_sentences

    d, tok = mode_tok
    sents = M.compound_sentences()
    utf8, offs = pack_sentences(sents)
    want = _got(tok, sents, "extended")
    T, n = len(want[0]), len(sents)
    opts = mode_opts("extended")

    def raw(tcap, opts=opts):
        tokens = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8)
        toff, costs, status = np.full(n + 1, 7, dtype=np.uint64), np.full(n, 7, dtype=np.int32), np.full(n, 0xEE, dtype=np.uint8)
        nt = C.c_uint64(0)
        rc = _lib.lib().kgpu_tokenize_batch_mode(tok.handle, utf8.ctypes.data, offs.ctypes.data, n, C.byref(opts), tokens.ctypes.data, tcap, toff.ctypes.data,
                                                 costs.ctypes.data, status.ctypes.data, C.byref(nt))
        return rc, tokens, toff, costs, status, nt.value

    rc, tokens, _, _, status, t = raw(T - 1)
    assert rc == _lib.KGPU_ERR_CAPACITY and t == T and not status.any() and (tokens == 0x5A).all()   # no record written
    rc, tokens, toff, costs, status, t = raw(T)
    assert rc == _lib.KGPU_OK and t == T
    assert tokens[: T * 24].view(TOKEN_DTYPE).tobytes() == want[0].tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert toff.tolist() == want[1].tolist() and costs.tolist() == want[2].tolist()
    with pytest.raises(_lib.KgpuError) as e:
        tok.tokenize_mode_packed(utf8, offs, "extended", token_capacity=T - 1)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY
    assert raw(T, _lib.ModeOpts(3, 2, 3000, 7, 1700))[0] == _lib.KGPU_ERR_INVALID_ARG
    bad = mode_opts("search")
    bad.reserved[0] = 1
    assert raw(T, bad)[0] == _lib.KGPU_ERR_INVALID_ARG


def test_synthetic_corpus(synth_tok):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok = synth_tok
    sents = synth.make_corpus(sd, 300, 51, "cfg2")
    utf8, offs = pack_sentences(sents)
    t1, toff1, st1 = tok.tokenize_packed(utf8, offs)
    tokens, toff, costs, status = tok.tokenize_mode_packed(utf8, offs, "normal")
    assert not status.any() and not st1.any()
    assert tokens.tobytes() == t1.tobytes() and toff.tolist() == toff1.tolist()   # NORMAL is tokenize, record for record
    want = _want(tok, sd.dict, sents, "search")
    _equal(_got(tok, sents, "search"), want)
    # (this corpus has no word long enough for the default penalties: lengths of 1 bite, and then SEARCH is no longer tokenize)
    tight = _want(tok, sd.dict, sents, "search", (1, 3000, 1, 1700))
    _equal(_got(tok, sents, "search", (1, 3000, 1, 1700)), tight)
    assert tight[0].tobytes() != t1.tobytes()
    # the Python class: Token objects, those of tokenize_batch in normal mode
    assert tok.tokenize_mode(sents[:3] + [""], "normal") == tok.tokenize_batch(sents[:3] + [""])
    rows = tok.tokenize_mode(sents[:3], "search")
    assert [[t.surface for t in r] for r in rows] == [_surfaces(s, want[0][int(want[1][i]) : int(want[1][i + 1])]) + ["EOS"] for i, s in enumerate(sents[:3])]


def test_cli_mode(mode_tok, tmp_path):
    from kanpyo_amd.dictfile import DictFile, MorphFeatureTable, save_dict

    d, tok = mode_tok
    sents = [M.KANJI_COMPOUND, M.compound_sentences()[3], "東京", "大阪府"]
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(M.mode_words()) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, 4)])
    path = tmp_path / "m.dict"
    save_dict(DictFile(d, known, unk), str(path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    data = "".join(s + "\n" for s in sents).encode()

    def run(extra):
        return subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)] + extra, input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)

    plain, normal, search = run([]), run(["--mode", "normal"]), run(["--mode", "search"])
    assert plain.returncode == 0 and normal.returncode == 0 and search.returncode == 0, (plain.stderr, normal.stderr, search.stderr)
    assert normal.stdout == plain.stdout and plain.stdout.count(b"EOS\t\n") == len(sents)
    lines = search.stdout.decode("utf-8").split("\n")
    heads = [ln.split("\t")[0] for ln in lines if ln]
    assert heads[:4] == list(M.KANJI_PARTS) + ["EOS"] and M.KANJI_COMPOUND not in heads and M.KANA_COMPOUND not in heads
    assert heads[-5:] == ["東京", "EOS", "大", "阪府", "EOS"] and M.KANJI_COMPOUND in plain.stdout.decode("utf-8")
    extended = run(["--mode", "extended", "--normalize", "nfkc"])
    assert extended.returncode == 0 and extended.stdout.decode("utf-8").count("\n") == search.stdout.decode("utf-8").count("\n") + 2 + 1   # ぬねの and ぬね cut up
    bad = run(["--mode", "search", "--split", "device"])
    assert bad.returncode == 2 and bad.stdout == b""
