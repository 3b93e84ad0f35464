"""The user dictionary on the device (include/kanpyo_gpu.h, "user dictionary"): kgpu_userdict_create, kgpu_tokenize_batch_user,
Tokenizer.tokenize_user* and `python -m kanpyo_amd tokenize --user-dict`.  The device must equal kgpu_userdict_host applied to kgpu_lattice_dump of the
same sentence, byte for byte: records, tok_offsets, costs and status.  The host function itself is pinned to a plain restatement, to brute force and
to a dictionary that holds the entries among its own words in tests/test_userdict_cpu.py; the dump is compared with the naive restatement's lattice node
for node, and this call with the host rule over the restatement's lattices (the withdrawal decisions where the invoke flag decides among them), in
tests/test_gpu_lattice_sweep.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mode_cases as M
import userdict_cases as U
from conftest import ROOT, fixture_dict_parts

pytestmark = pytest.mark.gpu

INF, NO_SCRATCH = 1 << 30, 2


def _tok(d):
    from kanpyo_amd import Tokenizer, _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return Tokenizer(d)


def _want(tok, d, sents, entries, mode, penalties=None):
    """kgpu_userdict_host over kgpu_lattice_dump, sentence after sentence (each distinct one once) -> the arrays of the batch call (a sentence given
    as bytes is not UTF-8: no records, cost 1 << 30, status 1)."""
    from kanpyo_amd.lattice import dump_lattice
    from kanpyo_amd.nbest import connection_matrix
    from kanpyo_amd.tokenizer import TOKEN_DTYPE
    from kanpyo_amd.userdict import userdict_host

    conn = connection_matrix(d)
    tokens, toff, costs, status, seen = [], [0], [], [], {}
    for s in sents:
        if isinstance(s, bytes):
            toff.append(toff[-1])
            costs.append(INF)
            status.append(1)
            continue
        if s not in seen:
            seen[s] = userdict_host(dump_lattice(tok, s), s, conn, d, entries, mode, penalties)
        t, c = seen[s]
        tokens.append(t)
        toff.append(toff[-1] + len(t))
        costs.append(c)
        status.append(0)
    return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(toff, dtype=np.uint64), np.array(costs, dtype=np.int32),
            np.array(status, dtype=np.uint8))


def _got(tok, ud, sents, mode, penalties=None):
    from kanpyo_amd.tokenizer import pack_sentences

    return tok.tokenize_user_packed(*pack_sentences(sents), ud, mode, penalties)


def _equal(got, want, what=""):
    for name, g, w in zip(("tokens", "tok_offsets", "costs", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def _both(tok, d, sents, entries, modes=M.MODES, penalties=None, what=""):
    """The device against the host rule for these entries in these modes -> {mode: the device's arrays}."""
    from kanpyo_amd import UserDict

    ud = UserDict(tok, entries)
    out = {}
    for mode in modes:
        out[mode] = _got(tok, ud, sents, mode, penalties)
        _equal(out[mode], _want(tok, d, sents, entries, mode, penalties), (what, mode))
    ud.close()
    return out


def _user_spans(got, i) -> list:
    t = got[0][int(got[1][i]) : int(got[1][i + 1])]
    return [(int(r["id"]), int(r["start"]), int(r["end"])) for r in t if int(r["cls"]) == 3]


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
def ascii_tok():
    d = U.ascii_dict()
    return d, _tok(d)


def test_fixture_and_mode_sentences(fixture_tok, mode_tok):
    rng = random.Random(5)
    d, tok = fixture_tok
    sents = M.FIXTURE_INPUTS
    entries = [e for s in sents for e in U.entries_from(rng, s, 2, [-200, 0, 3000], nctx=1)]
    got = _both(tok, d, sents, entries)
    assert any(_user_spans(got["normal"], i) for i in range(len(sents)))
    d, tok = mode_tok
    sents = M.compound_sentences() + M.threshold_sentences() + M.edge_sentences()
    entries = [(M.KANJI_COMPOUND, 0, 0, -100, ()), (M.FILLER, 1, 1, -500, ()), ("国際空港", 1, 0, 200, ()), ("東", 0, 0, 1, ()), ("京", 0, 1, 1, ())]
    got = _both(tok, d, sents, entries)
    assert _user_spans(got["normal"], 0) == [(1, 0, 6)] and _user_spans(got["search"], 0) == []   # the whole compound: taken, and penalised away
    for pen in ((3, 3000, 8, 1700), (0, 1, 0, 1)):
        _both(tok, d, sents, entries, ("search", "extended"), pen)


def test_no_entries_is_the_mode_call_and_tokenize(mode_tok):
    from kanpyo_amd import UserDict
    from kanpyo_amd.tokenizer import pack_sentences

    d, tok = mode_tok
    sents = M.compound_sentences() + M.threshold_sentences() + [""]
    ud = UserDict(tok, [])
    assert ud.info() == {"entries": 0, "keys": 0, "longest_key": 0, "device_bytes": 0}
    for mode in M.MODES:
        _equal(_got(tok, ud, sents, mode), tok.tokenize_mode_packed(*pack_sentences(sents), mode), mode)
    plain = tok.tokenize_packed(*pack_sentences(sents))
    got = _got(tok, ud, sents, "normal")
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tolist() == plain[1].tolist()
    ud.close()


def test_key_positions_lengths_and_scripts(ascii_tok, mode_tok):
    d, tok = ascii_tok
    k64 = "k" * 64
    sents = ["abcde", "xabcde", "abcdex", "ab", "abcabcabc", k64, k64 + k64[:10], "q" + k64, "a", "𠀀𠀁x𠀀𠀁", "x𠀀"]
    entries = [("ab", 0, 0, 5, ()), ("de", 1, 1, 5, ()), ("abcde", 0, 1, 7, ()), ("abcdef", 0, 0, 1, ()), ("a", 1, 0, 2, ()), (k64, 0, 0, 9, ()), ("𠀀𠀁", 1, 1, 3, ()),
               ("𠀀", 0, 0, 4, ()), ("abc", 0, 0, 1, ()), ("bca", 1, 1, 1, ()), ("cab", 0, 1, 1, ())]
    got = _both(tok, d, sents, entries)["normal"]
    # what the host rule gives, worked out once: the key that is the whole sentence; a key at the first characters (and none at the last: the unknown
    # word over the rest is cheaper); a 1-character key; the 64-character key alone and with ten characters behind it, not with one in front
    spans = [_user_spans(got, i) for i in range(len(sents))]
    assert spans[0] == [(3, 0, 5)] and spans[2] == [(1, 0, 2)] and spans[3] == [(1, 0, 2)] and spans[8] == [(5, 0, 1)]
    assert spans[4] == [(9, 0, 3), (9, 3, 6), (9, 6, 9)] and spans[5] == [(6, 0, 64)] == spans[6] and spans[7] == [] and spans[9] == [(8, 0, 1)]
    assert all(e != 4 for sp in spans for e, _, _ in sp)      # "abcdef" is longer than what is left of every sentence
    # overlapping matches all exist: ああ in あああ twice, and a key equal to a system word loses the tie to it
    d, tok = mode_tok
    word, m = "東京", dict(zip(sorted(M.mode_words(), key=lambda w: w.encode("utf-8")), range(10**6)))
    i = m[word]
    same = (word, i % 2, (i // 2) % 2, M.mode_words()[word], ())   # the morph mode_cases._from_words gives the word
    got = _both(tok, d, [word, word + word, "ぬ" + word], [same])
    assert all(_user_spans(got[mode], k) == [] for mode in M.MODES for k in range(3))
    cheaper = (word, same[1], same[2], same[3] - 1, ())
    assert _user_spans(_both(tok, d, [word], [cheaper])["normal"], 0) == [(1, 0, 2)]


def test_overlaps_and_shared_keys():
    """ああ in あああ matches twice; 65 entries share one key (more than one round of lanes over the user predecessors of the next position); and
    あ x 1025 with the key ああ has more user nodes than a forward workgroup has threads."""
    from nbest_cases import _dict

    d = _dict(["あ"], [(0, 1, 50)], 2, [0, 3, -2, 1], "あ", 0)
    tok = _tok(d)
    got = _both(tok, d, ["あああ", "ああ", "あ"], [("ああ", 1, 0, 60, ()), ("あああ", 0, 0, 500, ())])
    shared = [("ああ", k % 2, (k // 2) % 2, 90 + (k * 7) % 5, ()) for k in range(65)] + [("あ", 0, 0, 49, ())]
    got = _both(tok, d, ["ああああああ", "あああ"], shared)
    assert any(_user_spans(got[m], 0) for m in M.MODES)
    # three groups at every position with their entries interleaved and every cost equal: which node wins a tie is its rank by entry
    woven = [(("あ", "ああ", "あああ")[(k * 5) % 3], 0, 1, 40, ()) for k in range(90)]
    got = _both(tok, d, ["あああああ", "あああ", "ああ"], woven)
    assert {e for m in M.MODES for i in range(3) for e, _, _ in _user_spans(got[m], i)} <= {1, 2, 3}   # (the first entry of each key)
    long_ = "あ" * 1025
    got = _both(tok, d, [long_, "あ", long_[:300]], [("ああ", 1, 0, 60, ())], ("normal", "search"))
    assert len(_user_spans(got["normal"], 0)) >= 500
    tok.close()


def test_the_tables_worst_cases(ascii_tok):
    """Keys with one full hash (the bytes must decide), 24 keys of one home slot in a 64-slot table (a chain that wraps), keys that share every character but
    the last -- each as an entry, in sentences made of them."""
    from kanpyo_amd import UserDict

    d, tok = ascii_tok
    worst = U.table_worst_keys()
    rng = random.Random(9)
    for name, keys in worst.items():
        entries = [(k, i % 2, (i // 3) % 2, 10 + i, ()) for i, k in enumerate(keys)]
        sents = U.sentences_over(keys, rng, 12) + ["".join(keys)]
        got = _both(tok, d, sents, entries, ("normal",), what=name)["normal"]
        ids = {e for i in range(len(sents)) for e, _, _ in _user_spans(got, i)}
        assert len(ids) >= len(keys) * 3 // 4, (name, len(ids))
    # half of each colliding pair listed, the other half in the text: a hit that is none
    col = worst["colliding"]
    listed, absent = col[0::2], col[1::2]
    got = _both(tok, d, absent + listed, [(k, 0, 0, 1, ()) for k in listed], ("normal",))["normal"]
    assert all(_user_spans(got, i) == [] for i in range(len(absent))) and all(_user_spans(got, len(absent) + i) for i in range(len(listed)))
    ud = UserDict(tok, [(k, 0, 0, 1, ()) for k in worst["crowded"] + col[:8]])
    assert ud.info()["keys"] == 32 and ud.info()["entries"] == 32 and ud.info()["longest_key"] == 8 and ud.info()["device_bytes"] > 0
    ud.close()


def test_tie_dictionaries():
    rng = random.Random(78)
    users = 0
    for seed in range(8):   # 8 dictionaries x 25 sentences, each in the three modes
        d = M.tie_dict(3000 + seed)
        tok = _tok(d)
        sents = [M.tie_sentence(rng) for _ in range(25)]
        entries = [e for s in sents[:6] for e in U.entries_from(rng, s, 2, [0, 100])]
        pen = M.tie_penalties(rng)
        got = _both(tok, d, sents, entries, penalties=pen, what=seed)
        users += sum(bool(_user_spans(got["normal"], i)) for i in range(25))
        tok.close()
    assert users >= 20


def test_invalid_utf8_and_an_empty_sentence_in_the_middle(mode_tok):
    d, tok = mode_tok
    sents = [M.KANJI_COMPOUND, b"\xe3\x81", "", M.KANA_COMPOUND, b"\xff", M.FILLER]
    got = _both(tok, d, sents, [(M.FILLER, 0, 0, 1, ()), ("関西", 1, 1, 2, ())])
    for mode in M.MODES:
        g = got[mode]
        assert g[3].tolist() == [0, 1, 0, 0, 1, 0] and g[1][1] == g[1][2] and g[1][3] - g[1][2] == 1 and g[2][1] == INF


def test_1025_sentences_cross_the_chunk(mode_tok, monkeypatch):
    from kanpyo_amd import UserDict

    d, tok = mode_tok
    words = [M.KANJI_COMPOUND, M.KANA_COMPOUND, "東京", "大阪府", M.FILLER, "空港"]
    sents = [words[(i * 7 + i // 5) % len(words)] for i in range(1025)]
    entries = [(M.FILLER, 0, 0, 1, ()), ("関西国際", 1, 1, 2, ()), ("ウェアエンジニア", 0, 1, 3, ())]
    monkeypatch.delenv("KGPU_HOST_USER_CHUNK_SENTS", raising=False)
    ud = UserDict(tok, entries)
    for mode in ("normal", "search"):
        one = _got(tok, ud, sents, mode)
        _equal(one, _want(tok, d, sents, entries, mode))
        monkeypatch.setenv("KGPU_HOST_USER_CHUNK_SENTS", "3")
        _equal(_got(tok, ud, sents, mode), one, mode)
        monkeypatch.delenv("KGPU_HOST_USER_CHUNK_SENTS")
    ud.close()


def test_arena_protocol(fixture_tok, monkeypatch):
    """The kept lattices and their slabs outgrow the arena: the chunk runs again on a doubled one (KGPU_HOST_USER_ARENA_INITIAL bounds the first); at
    the largest arena (KGPU_HOST_USER_ARENA_MAX) the chunk is halved until the sentence that alone does not fit is left with KGPU_SENT_NO_SCRATCH and
    no records, its neighbours' records being what they always are."""
    from kanpyo_amd import UserDict

    d, tok = fixture_tok
    long_ = "辞書形態素あ" * 25
    sents = M.FIXTURE_INPUTS + [long_] + M.FIXTURE_INPUTS[::-1]
    entries = [("形態", 0, 0, 10, ()), ("あ", 0, 0, 10, ()), ("テ", 0, 0, 5, ())]
    ud = UserDict(tok, entries)
    want = _got(tok, ud, sents, "search")
    _equal(want, _want(tok, d, sents, entries, "search"))
    monkeypatch.setenv("KGPU_HOST_USER_ARENA_INITIAL", "2048")
    tok.routing(reset=True)
    _equal(_got(tok, ud, sents, "search"), want)   # regrows until everything fits
    assert tok.routing()["arena_regrows"] >= 3
    monkeypatch.setenv("KGPU_HOST_USER_ARENA_MAX", "8192")
    got = _got(tok, ud, sents, "search")
    assert got[3].tolist() == [0] * 6 + [NO_SCRATCH] + [0] * 6 and got[2][6] == INF
    short = [s for s in sents if s != long_]
    monkeypatch.delenv("KGPU_HOST_USER_ARENA_INITIAL")
    monkeypatch.delenv("KGPU_HOST_USER_ARENA_MAX")
    rest = _got(tok, ud, short, "search")
    assert got[1][6] == got[1][7] and got[0].tobytes() == rest[0].tobytes()
    assert np.delete(got[1], 7).tolist() == rest[1].tolist() and np.delete(got[2], 6).tolist() == rest[2].tolist()
    _equal(_got(tok, ud, sents, "search"), want)
    ud.close()


def test_capacity_one_short_and_refusals(mode_tok):
    from kanpyo_amd import UserDict, _lib
    from kanpyo_amd.mode import mode_opts
    from kanpyo_amd.tokenizer import TOKEN_DTYPE, pack_sentences

    d, tok = mode_tok
    sents = M.compound_sentences()
    utf8, offs = pack_sentences(sents)
    ud = UserDict(tok, [(M.FILLER[:2], 0, 1, -300, ()), (M.KANJI_PARTS[0], 1, 1, 10, ())])
    want = _got(tok, ud, sents, "extended")
    T, n = len(want[0]), len(sents)
    opts = mode_opts("extended")

    def raw(tcap, opts=opts, handle=None, null_opts=False):
        tokens = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8)
        toff, costs, status = np.full(n + 1, 7, dtype=np.uint64), np.full(n, 7, dtype=np.int32), np.full(n, 0xEE, dtype=np.uint8)
        nt = C.c_uint64(0)
        rc = _lib.lib().kgpu_tokenize_batch_user(tok.handle, handle or ud.handle, utf8.ctypes.data, offs.ctypes.data, n, None if null_opts else C.byref(opts), tokens.ctypes.data, tcap,
                                                 toff.ctypes.data, costs.ctypes.data, status.ctypes.data, C.byref(nt))
        return rc, tokens, toff, costs, status, nt.value

    rc, tokens, _, _, status, t = raw(T - 1)
    assert rc == _lib.KGPU_ERR_CAPACITY and t == T and not status.any() and (tokens == 0x5A).all()   # no record written
    rc, tokens, toff, costs, status, t = raw(T)
    assert rc == _lib.KGPU_OK and t == T
    assert tokens[: T * 24].view(TOKEN_DTYPE).tobytes() == want[0].tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert toff.tolist() == want[1].tolist() and costs.tolist() == want[2].tolist()
    with pytest.raises(_lib.KgpuError) as e:
        tok.tokenize_user_packed(utf8, offs, ud, "extended", token_capacity=T - 1)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY
    assert raw(T, _lib.ModeOpts(3, 2, 3000, 7, 1700))[0] == _lib.KGPU_ERR_INVALID_ARG
    rc, tokens, toff, _, _, t = raw(T, null_opts=True)     # NULL options: normal mode
    assert rc == _lib.KGPU_OK and tokens[: t * 24].view(TOKEN_DTYPE).tobytes() == _got(tok, ud, sents, "normal")[0].tobytes()
    # a handle of another dictionary, and entries the create call refuses
    other = _tok(M.long_dict())
    foreign = UserDict(other, [("東", 0, 0, 1, ())])
    assert raw(T, handle=foreign.handle)[0] == _lib.KGPU_ERR_INVALID_ARG
    foreign.close()
    other.close()
    for bad in ([("", 0, 0, 0)], [("x" * 65, 0, 0, 0)], [("𠀀" * 64, 0, 0, 0)], [(b"\xff", 0, 0, 0)], [("a", 2, 0, 0)], [("a", 0, 2, 0)]):
        with pytest.raises(_lib.KgpuError) as e:
            UserDict(tok, [("ok", 0, 0, 0)] + bad)
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG, bad
    ud.close()


def test_two_user_dictionaries_alternate(mode_tok):
    from kanpyo_amd import UserDict
    from kanpyo_amd.tokenizer import pack_sentences

    d, tok = mode_tok
    sents = M.compound_sentences() + ["東京", M.FILLER]
    ea, eb = [(M.KANJI_COMPOUND, 0, 0, -100, ("a",))], [(M.FILLER, 1, 1, -500, ("b",)), ("東京", 0, 0, -50, ("b2",))]
    ua, ub = UserDict(tok, ea), UserDict(tok, eb)
    wa, wb = _want(tok, d, sents, ea, "normal"), _want(tok, d, sents, eb, "normal")
    assert wa[0].tobytes() != wb[0].tobytes()
    packed = pack_sentences(sents)
    for _ in range(2):
        _equal(_got(tok, ua, sents, "normal"), wa)
        mode = tok.tokenize_mode_packed(*packed, "search")
        _equal(_got(tok, ub, sents, "normal"), wb)
        nbest = tok.tokenize_nbest_packed(*packed, 2)
    assert len(mode[0]) and len(nbest[0])
    rows = tok.tokenize_user(sents[-2:], ub)
    assert [(t.class_.name, t.surface) for t in rows[0]] == [("User", "東京"), ("Dummy", "EOS")] and ub.features(rows[0][0].id) == ["b2"]
    assert ub.features(rows[1][0].id) == ["b"] and ub.entry(rows[1][0].id).surface == M.FILLER
    ua.close()
    ub.close()


def test_cli_user_dict(mode_tok, tmp_path):
    from kanpyo_amd.dictfile import DictFile, MorphFeatureTable, save_dict

    d, tok = mode_tok
    sents = [M.KANJI_COMPOUND, M.FILLER + "東京", "ｶﾞ東京"]
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(M.mode_words()) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, 4)])
    path = tmp_path / "m.dict"
    save_dict(DictFile(d, known, unk), str(path))
    csv = tmp_path / "user.csv"
    csv.write_text(f"{M.KANJI_COMPOUND},0,0,-100,名詞,固有名詞,空港\n{M.FILLER},1,1,-500,感動詞\nｶﾞ,0,0,-500,助詞,half\n", encoding="utf-8")
    env = dict(os.environ, PYTHONPATH=ROOT)
    data = "".join(s + "\n" for s in sents).encode()

    def run(extra):
        return subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)] + extra, input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)

    plain, user = run([]), run(["--user-dict", str(csv)])
    assert plain.returncode == 0 and user.returncode == 0, (plain.stderr, user.stderr)
    out = user.stdout.decode("utf-8")
    assert out.startswith(f"{M.KANJI_COMPOUND}\t名詞,固有名詞,空港\nEOS\t\n{M.FILLER}\t感動詞\n東京\t名詞,") and out.count("EOS\t\n") == 3
    assert "ｶﾞ\t助詞,half\n" in out                                   # without --normalize the half-width key matches the half-width text
    search = run(["--user-dict", str(csv), "--mode", "search", "--normalize", "nfkc"])
    assert search.returncode == 0, search.stderr
    heads = [ln.split("\t")[0] for ln in search.stdout.decode("utf-8").split("\n") if ln]
    assert heads[:4] == list(M.KANJI_PARTS) + ["EOS"] and "ガ" in heads and "ｶﾞ" not in heads and "ガ\t助詞,half\n" in search.stdout.decode("utf-8")
    sentences = run(["--user-dict", str(csv), "--sentences"])
    assert sentences.returncode == 0 and sentences.stdout == user.stdout
    bad = run(["--user-dict", str(csv), "--split", "device"])
    assert bad.returncode == 2 and bad.stdout == b""
    broken = tmp_path / "broken.csv"
    broken.write_text("ok,0,0,0\nbroken,0\n", encoding="utf-8")
    bad = run(["--user-dict", str(broken)])
    assert bad.returncode == 2 and bad.stdout == b"" and b"line 2" in bad.stderr
