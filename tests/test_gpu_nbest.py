"""N-best paths on the device (include/kanpyo_gpu.h, "N-best paths"): kgpu_tokenize_batch_nbest, Tokenizer.tokenize_nbest* and
`python -m kanpyo_amd tokenize --nbest`.  The device must equal kgpu_nbest_host applied to kgpu_lattice_dump of the same sentence, byte for byte:
path_offsets, tok_offsets, costs, records and status.  The host function itself is pinned to a brute-force enumeration in tests/test_nbest_cpu.py;
the dump is compared with the naive restatement's lattice node for node, and this call with the host rule over the restatement's lattices, in
tests/test_gpu_lattice_sweep.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, fixture_dict_parts
from nbest_cases import CROWDED_SENTENCE, FIXTURE_INPUTS, crowded_dict, max_candidates, tie_dict, tie_sentence

pytestmark = pytest.mark.gpu

NO_SCRATCH = 2


def _tok(d):
    from kanpyo_amd import Tokenizer, _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return Tokenizer(d)


def _want(tok, d, sents, k, lats=None):
    """kgpu_nbest_host over kgpu_lattice_dump, sentence after sentence -> the arrays of the batch call (a sentence given as bytes is not UTF-8)."""
    from kanpyo_amd.lattice import dump_lattice
    from kanpyo_amd.nbest import connection_matrix, nbest_host
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    conn = connection_matrix(d)
    tokens, poff, toff, costs, status = [], [0], [0], [], []
    for s in sents:
        if isinstance(s, bytes):
            poff.append(poff[-1])
            status.append(1)
            continue
        lat = dump_lattice(tok, s)
        if lats is not None:
            lats.append(lat)
        t, o, c = nbest_host(lat, conn, k)
        tokens.append(t)
        toff += (o[1:].astype(np.int64) + toff[-1]).tolist()
        costs += c.tolist()
        poff.append(poff[-1] + len(c))
        status.append(0)
    return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(poff, dtype=np.uint64), np.array(toff, dtype=np.uint64),
            np.array(costs, dtype=np.int32), np.array(status, dtype=np.uint8))


def _got(tok, sents, k):
    from kanpyo_amd.tokenizer import pack_sentences

    return tok.tokenize_nbest_packed(*pack_sentences(sents), k)


def _equal(got, want, what=""):
    for name, g, w in zip(("tokens", "path_offsets", "tok_offsets", "costs", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


@pytest.fixture(scope="module")
def fixture_tok():
    from kanpyo_amd import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    return d, _tok(d)


@pytest.fixture(scope="module")
def synth_tok():
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=11)
    return sd, _tok(sd.dict)


@pytest.mark.parametrize("k", [1, 2, 64])
def test_fixture_sentences(fixture_tok, k):
    d, tok = fixture_tok
    got = _got(tok, FIXTURE_INPUTS, k)
    _equal(got, _want(tok, d, FIXTURE_INPUTS, k))
    counts = np.diff(got[1].astype(np.int64)).tolist()
    assert counts[0] == 1 and 0 in counts and not got[4].any()   # "": [EOS]; an unreachable EOS: no paths, status 0
    if k == 64:
        assert any(1 < c < 64 for c in counts)                   # fewer than k paths: all of them


def test_invalid_utf8_between_valid_sentences(fixture_tok):
    d, tok = fixture_tok
    sents = ["テスト", b"\xe3\x81", "あいうえお", b"\xff", ""]
    got = _got(tok, sents, 3)
    _equal(got, _want(tok, d, sents, 3))
    assert got[4].tolist() == [0, 1, 0, 1, 0] and got[1][1] == got[1][2] and got[1][3] == got[1][4]


@pytest.mark.parametrize("k", [3, 8])
def test_tie_dictionaries(k):
    rng = random.Random(100 + k)
    for seed in range(4):   # 4 dictionaries x 16 sentences
        d = tie_dict(1000 + seed)
        tok = _tok(d)
        sents = [tie_sentence(rng) for _ in range(16)]
        _equal(_got(tok, sents, k), _want(tok, d, sents, k), (seed, sents))
        tok.close()


@pytest.mark.parametrize("k", [16, 64])
def test_more_than_64_candidates_per_target(k):
    """More than one round of the forward kernel's selection: a crowded position, its predecessors' lists full."""
    d = crowded_dict()
    tok = _tok(d)
    sents = [CROWDED_SENTENCE, CROWDED_SENTENCE[::-1], "あ" * 9]
    lats = []
    want = _want(tok, d, sents, k, lats)
    widest, most = max_candidates(lats[0], k)
    assert widest > 8 and most > 64 * 2, (widest, most)
    got = _got(tok, sents, k)
    _equal(got, want)
    assert np.diff(got[1].astype(np.int64)).tolist() == [k] * 3
    tok.close()


def test_path_0_is_tokenize(synth_tok):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok = synth_tok
    sents = synth.make_corpus(sd, 256, 41, "cfg2")
    utf8, offs = pack_sentences(sents)
    t1, toff1, st1 = tok.tokenize_packed(utf8, offs)
    tokens, poff, toff, costs, status = tok.tokenize_nbest_packed(utf8, offs, 10)
    assert not status.any() and not st1.any()
    for i in range(len(sents)):
        p = int(poff[i])
        assert int(poff[i + 1]) > p
        assert tokens[int(toff[p]) : int(toff[p + 1])].tobytes() == t1[int(toff1[i]) : int(toff1[i + 1])].tobytes(), sents[i]
        c = costs[p : int(poff[i + 1])].astype(np.int64)
        assert (np.diff(c) >= 0).all()
    # ... and a sample of them against the host function
    _equal(_got(tok, sents[:24], 10), _want(tok, sd.dict, sents[:24], 10))
    # the Python class: Token objects, those of tokenize_batch on path 0
    paths = tok.tokenize_nbest(sents[:3] + [""], 4)
    assert [p[0].tokens for p in paths] == [tuple(r) for r in tok.tokenize_batch(sents[:3] + [""])]
    assert all(len(p) == 4 for p in paths[:3]) and len(paths[3]) == 1 and paths[0][0].cost == int(costs[0])


def test_one_long_sentence(synth_tok):
    """2048 characters with a groupable run past MAX_UNKNOWN_LEN (lattice.rs:55), between ordinary neighbours."""
    from kanpyo_amd import synth

    sd, tok = synth_tok
    around = synth.make_corpus(sd, 4, 42, "cfg2")
    long_ = (around[0] + "ア" * 1100 + around[1] + "ゞ" * 30 + around[2] * 40)[:2048]
    assert len(long_) == 2048
    sents = [around[3], long_, around[0]]
    _equal(_got(tok, sents, 4), _want(tok, sd.dict, sents, 4))


def test_chunking_gives_the_same_arrays(synth_tok, monkeypatch):
    from kanpyo_amd import synth

    sd, tok = synth_tok
    sents = synth.make_corpus(sd, 20, 43, "cfg2") + ["", b"\xff"] + synth.make_corpus(sd, 8, 44, "cfg3")
    monkeypatch.delenv("KGPU_HOST_NBEST_CHUNK_SENTS", raising=False)
    one = _got(tok, sents, 5)
    _equal(one, _want(tok, sd.dict, sents, 5))
    for m in ("1", "7"):
        monkeypatch.setenv("KGPU_HOST_NBEST_CHUNK_SENTS", m)
        _equal(_got(tok, sents, 5), one, m)
    monkeypatch.delenv("KGPU_HOST_NBEST_CHUNK_SENTS")


def test_arena_protocol(fixture_tok, monkeypatch):
    """The kept lattices and their lists outgrow the arena: the chunk runs again on a doubled one (KGPU_HOST_NBEST_ARENA_INITIAL bounds the first); at
    the largest arena (KGPU_HOST_NBEST_ARENA_MAX) the chunk is halved until the sentence that alone does not fit is left with KGPU_SENT_NO_SCRATCH and
    no paths, its neighbours' paths being what they always are."""
    d, tok = fixture_tok
    long_ = "辞書形態素あ" * 25
    sents = FIXTURE_INPUTS + [long_] + FIXTURE_INPUTS[::-1]
    want = _got(tok, sents, 8)
    _equal(want, _want(tok, d, sents, 8))
    monkeypatch.setenv("KGPU_HOST_NBEST_ARENA_INITIAL", "2048")
    tok.routing(reset=True)
    _equal(_got(tok, sents, 8), want)   # regrows until everything fits
    assert tok.routing()["arena_regrows"] >= 3
    monkeypatch.setenv("KGPU_HOST_NBEST_ARENA_MAX", "8192")
    got = _got(tok, sents, 8)
    assert got[4].tolist() == [0] * 6 + [NO_SCRATCH] + [0] * 6
    short = [s for s in sents if s != long_]
    monkeypatch.delenv("KGPU_HOST_NBEST_ARENA_INITIAL")
    monkeypatch.delenv("KGPU_HOST_NBEST_ARENA_MAX")
    rest = _got(tok, short, 8)
    assert got[1][6] == got[1][7] and got[0].tobytes() == rest[0].tobytes() and got[2].tobytes() == rest[2].tobytes() and got[3].tobytes() == rest[3].tobytes()
    assert np.delete(got[1], 7).tolist() == rest[1].tolist()
    _equal(_got(tok, sents, 8), want)


def test_capacity_one_short(fixture_tok):
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import TOKEN_DTYPE, pack_sentences

    d, tok = fixture_tok
    utf8, offs = pack_sentences(FIXTURE_INPUTS)
    want = _got(tok, FIXTURE_INPUTS, 4)
    T, P, n = len(want[0]), len(want[3]), len(FIXTURE_INPUTS)

    def raw(tcap, pcap):
        tokens, toff, costs = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8), np.full(pcap + 3, 7, dtype=np.uint64), np.full(pcap + 2, 7, dtype=np.int32)
        poff, status = np.zeros(n + 1, dtype=np.uint64), np.full(n, 0xEE, dtype=np.uint8)
        np_, nt = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().kgpu_tokenize_batch_nbest(tok.handle, utf8.ctypes.data, offs.ctypes.data, n, 4, tokens.ctypes.data, tcap, poff.ctypes.data, toff.ctypes.data,
                                                  costs.ctypes.data, pcap, status.ctypes.data, C.byref(np_), C.byref(nt))
        return rc, tokens, poff, toff, costs, status, np_.value, nt.value

    for tcap, pcap in ((T, P - 1), (T - 1, P)):   # one path short, one token short
        rc, tokens, _, toff, costs, status, p, t = raw(tcap, pcap)
        assert rc == _lib.KGPU_ERR_CAPACITY and (p, t) == (P, T) and not status.any()
        assert (tokens == 0x5A).all() and (costs == 7).all() and (toff[1:] == 7).all()   # one chunk: nothing written
    rc, tokens, poff, toff, costs, status, p, t = raw(T, P)
    assert rc == _lib.KGPU_OK and (p, t) == (P, T)
    assert tokens[: T * 24].view(TOKEN_DTYPE).tobytes() == want[0].tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert poff.tolist() == want[1].tolist() and toff[: P + 1].tolist() == want[2].tolist() and costs[:P].tolist() == want[3].tolist()
    assert (toff[P + 1 :] == 7).all() and (costs[P:] == 7).all()
    for k in (0, 65):
        with pytest.raises(_lib.KgpuError) as e:
            _got(tok, FIXTURE_INPUTS, k)
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG


def test_routing_counters_of_a_plain_call_are_untouched(synth_tok):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok = synth_tok
    utf8, offs = pack_sentences(synth.make_corpus(sd, 64, 45, "cfg2"))

    def plain():
        before = tok.routing()
        res = [a.copy() for a in tok.tokenize_packed(utf8, offs)]
        after = tok.routing()
        return res, {n: (np.array(after[n]) - np.array(before[n])).tolist() for n in after if n != "first_ms"}

    plain()   # (the first call of a handle creates its pooled context)
    r0, d0 = plain()
    _got(tok, synth.make_corpus(sd, 32, 46, "cfg2"), 5)
    r1, d1 = plain()
    assert d0 == d1
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b)


def test_cli_nbest(fixture_tok, tmp_path):
    from conftest import load_golden
    from kanpyo_amd.dictfile import DictFile, MorphFeatureTable, save_dict
    from kanpyo_amd.lattice import dump_lattice
    from kanpyo_amd.nbest import nbest_host, path_lines

    d, tok = fixture_tok
    g = load_golden("fixture_graphviz.json")
    p = fixture_dict_parts()
    known = MorphFeatureTable.from_features([g["features"]["known"].get(str(i), ["名詞", f"k{i}", "*"]) for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([g["features"]["unknown"][str(i)] for i in range(1, len(p["unk_morphs"]) + 1)])
    path = tmp_path / "t.dict"
    save_dict(DictFile(d, known, unk), str(path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    lines = [s for s in FIXTURE_INPUTS if s] + [g["input"]]
    data = "".join(s + "\n" for s in lines).encode()

    def run(extra):
        return subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)] + extra, input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)

    plain, one, three = run([]), run(["--nbest", "1"]), run(["--nbest", "3"])
    assert plain.returncode == 0 and one.returncode == 0 and three.returncode == 0, (plain.stderr, one.stderr, three.stderr)
    # --nbest 1 is `tokenize` on every line whose EOS is reachable; the others print nothing with --nbest (there is no real path)
    reachable = [s for s in lines if len(nbest_host(dump_lattice(tok, s), d, 1)[2])]
    assert len(reachable) >= 3
    assert one.stdout == subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)], input="".join(s + "\n" for s in reachable).encode(),
                                        capture_output=True, env=env, cwd=ROOT, timeout=600).stdout
    if len(reachable) == len(lines):
        assert one.stdout == plain.stdout
    want = b""
    for s in lines:
        t, o, c = nbest_host(dump_lattice(tok, s), d, 3)
        want += b"".join(path_lines(s.encode(), t[int(o[q]) : int(o[q + 1])], known, unk) for q in range(len(c)))
    assert three.stdout == want and three.stdout.count(b"EOS\t\n") > len(reachable)
    bad = run(["--nbest", "2", "--split", "device"])
    assert bad.returncode == 2 and bad.stdout == b""
