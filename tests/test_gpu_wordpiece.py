"""The WordPiece ids on the device (include/kanpyo_gpu.h, "WordPiece ids"; kgpu_wordpiece.hip): a WordPiece vocabulary through kgpu_encode_batch,
kgpu_encode_text, kgpu_encode_device ragged and padded, Vocab.encode_tensor and `python -m kanpyo_amd encode --wordpiece`.  Expected values
always come from the oracle's tokens (or crafted records) through tests/wordpiece_ref.py, or from tests/golden/fixture_wordpiece.json -- never
from the library.  No tolerance: ids and all n + 1 offsets are compared exactly.  The fixtures follow tests/test_gpu_encode.py's pattern."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import encode_ref as E
import lines_ref as R
import wordpiece_ref as WP
from conftest import ROOT, load_golden
from record_cases import SENTINEL, SMALL_KEYS, SPECIALS, _Dev, _Env, bert_like, check_ragged, corpus_of, dev_encode, env, ref_spec, same, small_ctx  # noqa: F401
from record_cases import plain_small_env as small_env  # noqa: F401  (env, small_ctx, small_env: the fixtures; this small_env has every EOS reachable)

pytestmark = pytest.mark.gpu

U, K = R.UNKNOWN, R.KNOWN


@pytest.fixture(scope="module")
def mixed(env):
    """1500 keyed, 600 cfg 2 and 100 cfg 3 sentences, packed, with the oracle's tokens, their words and the BERT-like list: computed once, never changed."""
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(corpus_of(env.sd, env.keys, 1500, 600, 100, 7))
    exp = env.orc.tokenize_batch(utf8, offs, 8)
    words = E.sentence_words(utf8, offs, exp.tokens, exp.offsets, env.known, env.unk, env.nk, env.nu, ref_spec(), env.keys)
    return utf8, offs, (exp.tokens, exp.offsets), words, bert_like(words, 500)


def ref_ids(env, utf8, offs, vocab, unk, bos=None, eos=None, tokens=None, kw=None, stats=None, **wp):
    if tokens is None:
        exp = env.orc.tokenize_batch(utf8, offs, 8)
        tokens = (exp.tokens, exp.offsets)
    return WP.encode(utf8, offs, *tokens, env.known, env.unk, env.nk, env.nu, ref_spec(**(kw or {})), env.keys, vocab, unk, bos, eos, stats=stats, **wp)


def crafted_ids(env, case, vocab, unk, bos=None, eos=None, kw=None, **wp):
    return WP.encode(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**(kw or {})), SMALL_KEYS, vocab, unk, bos, eos, **wp)


# ---- 1. the golden file ---------------------------------------------------------------------------------------------------------------------------
def test_golden_file_host_form_and_device_form(small_env, small_ctx):
    g = load_golden("fixture_wordpiece.json")
    # the fixture dictionary: テスト is a known token (its row holds the pieces), あいうえお an unknown one (matched in the text); one list for both
    f = g["fixture_dict"]
    vocab = [WP.golden_bytes(x) for x in f["list"]]
    unk = vocab.index(WP.golden_bytes(f["unk"]))
    want = [[vocab.index(WP.golden_bytes(p)) for p in row] for row in f["pieces"]]
    v = small_env.words().vocabulary(vocab, unk, wordpiece=True)
    assert [a.tolist() for a in v.encode(f["sentences"])] == want
    exp = small_env.orc.tokenize_batch(*_packed(f["sentences"]), 8)
    real = [(int(t["cls"]), int(t["id"]), int(t["byte_len"])) for t in exp.tokens if t["cls"] != R.DUMMY]
    assert real[0] == (K, 1, 9) and real[1][0] == U and real[1][2] == 15, "テスト is known by its row, あいうえお unknown by its text"
    info, wi = v.info(), v.wordpiece_info()
    assert info["n_words"] == len(vocab) and info["table_slots"] == 32 and wi["cont_words"] == 6 and wi["cont_table_slots"] == 16
    assert (wi["rows_whole"], wi["rows_split"], wi["rows_unk"], wi["row_piece_ids"]) == (0, 1, 2, 2) and (wi["max_initial_bytes"], wi["max_cont_bytes"]) == (8, 6)
    assert [a.tolist() for a in v.split_words(["テスト", "あいうえお", ""])] == want[:2] + [[]]
    v.close()
    # every case of the file: its words as unknown-class records without a row over a text that holds them back to back (device form), and as
    # sentences of their own through kgpu_encode_batch with the oracle's tokens (valid UTF-8 words only)
    for c in g["cases"]:
        vocab = [WP.golden_bytes(x) for x in c["list"]]
        unk, prefix = vocab.index(WP.golden_bytes(c["unk"])), WP.golden_bytes(c["prefix"])
        words = [WP.golden_bytes(w["word"]) for w in c["words"]]
        want = [[vocab.index(p) for p in WP.golden_pieces(w["pieces"])] for w in c["words"]]
        text, recs, at = b"".join(words), [], 0
        for w in words:
            recs.append((0, U, at, len(w)))
            at += len(w)
        case = R.pack([text, text], [recs, recs[::-1]])
        flat = [i for row in want for i in row]
        back = [i for row in want[::-1] for i in row]
        expect = (np.array(flat + back, dtype=np.int32), np.array([0, len(flat), 2 * len(flat)], dtype=np.uint64))
        same(crafted_ids(small_env, case, vocab, unk, prefix=prefix, max_chars=c["max_chars"]), expect, c["name"])   # (the reference agrees with the file)
        v = small_env.words().vocabulary(vocab, unk, wordpiece=True, prefix=prefix, max_word_chars=c["max_chars"])
        check_ragged(small_ctx, v, case, expect)
        sents = []
        for w in words:
            try:
                sents.append(w.decode("utf-8"))
            except UnicodeDecodeError:
                pass
        utf8, offs = _packed(sents)
        ids, ioff, st = v.encode_packed(utf8, offs)
        assert not st.any()
        same((ids, ioff), ref_ids(small_env_keys(small_env), utf8, offs, vocab, unk, prefix=prefix, max_chars=c["max_chars"]), c["name"])
        v.close()


def _packed(sents):
    from kanpyo_amd.tokenizer import pack_sentences

    return pack_sentences(sents)


def small_env_keys(e):
    e.keys = SMALL_KEYS
    return e


# ---- 2. crafted records: windows, counts of 0 / 1 / 2 / 10 / 100, padded cuts ----------------------------------------------------------------------
TEXT = b"ab" + b"c" * 100 + b"zq" + "テスト辞書".encode()   # a | ab | c x 100 | zq | テスト | 辞書
KINDS = {   # (id, class, position, byte_len): what a record of the kind is
    "empty": (1, U, 0, 0),          # an empty unknown-class surface: no id
    "one": (1, U, 0, 1),            # "a": listed
    "two": (0, U, 0, 2),            # "ab": a ##b (a record without a row)
    "hundred": (1, U, 2, 100),      # c ##c x 99
    "unk": (1, U, 102, 2),          # "zq": no piece starts with z
    "row2": (1, K, 3, 1),           # known id 1: its key テスト -> テ ##スト from the pool, whatever its surface says
    "row1": (2, K, 0, 0),           # known id 2: 辞書, listed whole
    "rowunk": (3, K, 0, 0),         # known id 3: 形態素, not listed
    "text2": (0, U, 104, 9),        # the bytes テスト as an unknown record: matched in the text
}
CRAFT_LIST = SPECIALS + [b"a", b"##b", b"c", b"##c", "テ".encode(), "##スト".encode(), "辞書".encode(), "名".encode(), "##名".encode(), "未知".encode()]
LENGTHS = (1, 63, 64, 65, 128, 129)
FILL = ("one", "row1", "two", "unk", "row2")


def crafted_case(special):
    """One sentence per length of LENGTHS: `special` on lanes 0 and 63 and on the first lane of the next window, a rotating mix elsewhere."""
    per = []
    for T in LENGTHS:
        per.append([KINDS[special if k in (0, 63, 64) else FILL[(k + T) % len(FILL)]] for k in range(T)])
    return R.pack([TEXT] * len(LENGTHS), per)


def cut_kinds(case, env, vocab, unk, bos, width, kw):
    """Where a row of `width` is cut, by the reference: "between" tokens or "inside" a token's pieces, per sentence that is cut at all."""
    words = E.sentence_words(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), SMALL_KEYS)
    tabs = WP.tables(vocab)
    kinds = set()
    for s in words:
        ends, at = set(), 1 if bos is not None else 0
        for w in s:
            at += len(WP.split_with(tabs, w, 100, unk))
            ends.add(at)
        if at > width:
            kinds.add("between" if width in ends or width <= (bos is not None) else "inside")
    return kinds


@pytest.mark.parametrize("special", ["empty", "one", "two", "hundred", "row2", "text2"])
def test_crafted_records_ragged_and_padded(small_env, small_ctx, special):
    case = crafted_case(special)
    dcase = _Dev(case)
    n = dcase.n
    for kw in ({}, {"field": 0}):   # field 0: known id 2 is "名" x 10 -> ten pieces from the pool, id 3 a 3400-character name -> [UNK], unknown ids "未知"
        seen = set()
        for bos, eos in ((None, None), (2, 3)):
            want = crafted_ids(small_env, case, CRAFT_LIST, 1, bos, eos, kw)
            L = np.diff(want[1].astype(np.int64))
            per_token = {"empty": 0, "one": 1, "two": 2, "hundred": 100, "row2": 2, "text2": 2}[special]
            if not kw:
                assert L[0] == per_token + (bos is not None) + (eos is not None), "a sentence of one record gives its pieces"
            v = small_env.words(**kw).vocabulary(CRAFT_LIST, 1, bos, eos, wordpiece=True)
            check_ragged(small_ctx, v, dcase, want)
            for width in (1, 2, 3, 64, 65, 101, 130, 400):
                ref = WP.padded(want[0], want[1], width, -9, eos)
                seen |= cut_kinds(case, small_env, CRAFT_LIST, 1, bos, width - (eos is not None), kw)
                rc, got, buf, ioff = dev_encode(small_ctx, v, dcase, width=width, pad_id=-9, capacity=n * width, room=n * width + 48)
                assert (rc, got) == (0, len(want[0])), (special, width)
                assert np.array_equal(ioff, want[1]), "id_offsets of the padded form are the ragged run's"
                assert np.array_equal(buf[: n * width].reshape(n, width), ref), (special, width, bos, kw)
                assert (buf[n * width :] == SENTINEL).all(), "ids behind n x width"
            v.close()
        assert seen == {"between", "inside"}, "rows cut between tokens and inside a token's pieces"
    if special == "hundred":
        want = crafted_ids(small_env, case, CRAFT_LIST, 1)
        assert int(np.diff(want[1].astype(np.int64)).max()) > 300 and want[0].tolist()[:100] == [6] + [7] * 99


def test_the_same_bytes_as_a_known_and_as_an_unknown_token(small_env, small_ctx):
    text = "テスト辞書形態素".encode()
    recs = [(1, K, 0, 9), (0, U, 0, 9), (1, U, 0, 9), (2, K, 9, 6), (0, U, 9, 6), (3, K, 15, 9), (0, U, 15, 9)]
    case = R.pack([text], [recs])
    for vocab in (CRAFT_LIST, CRAFT_LIST + ["形".encode(), "##態".encode(), "##素".encode()], SPECIALS + ["テスト".encode(), "##書".encode(), "辞".encode()]):
        want = crafted_ids(small_env, case, vocab, 1)
        rows = [WP.split(w, vocab, unk_id=1) for w in ("テスト", "辞書", "形態素")]
        assert want[0].tolist() == rows[0] * 3 + rows[1] * 2 + rows[2] * 2, "by the reference: the row table and the text match agree"
        v = small_env.words().vocabulary(vocab, 1, wordpiece=True)
        check_ragged(small_ctx, v, case, want)
        v.close()


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_device_and_host_forms(env, small_env, small_ctx):
    from kanpyo_amd import _lib

    case = crafted_case("hundred")
    want = crafted_ids(small_env, case, CRAFT_LIST, 1, 2, 3)
    total = len(want[0])
    v = small_env.words().vocabulary(CRAFT_LIST, 1, 2, 3, wordpiece=True)
    rc, got, buf, _ = dev_encode(small_ctx, v, case, capacity=total - 1, room=total + 8)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == total and (buf == SENTINEL).all(), "one below the total: the exact count, nothing written"
    rc, got, buf, _ = dev_encode(small_ctx, v, case, capacity=total, room=total + 8)
    assert (rc, got) == (0, total) and np.array_equal(buf[:total], want[0]) and (buf[total:] == SENTINEL).all()
    v.close()
    # the host form on a list of characters alone: latin runs are one token each and give an id per character, far more ids than records and more
    # than the chunk's first block holds ((bytes / 2 + 2 n + 1024) ids): the grow-and-rerun path
    rng = random.Random(3)
    sents = [" ".join("".join(rng.choice("abcdefgh") for _ in range(rng.randrange(4, 12))) for _ in range(60)) for _ in range(40)]
    utf8, offs = _packed(sents)
    chars = [c.encode() for c in "abcdefgh"]
    vocab = SPECIALS + chars + [b"##" + c for c in chars]
    exp = env.orc.tokenize_batch(utf8, offs, 8)
    want = ref_ids(env, utf8, offs, vocab, 1, tokens=(exp.tokens, exp.offsets))
    total, n = len(want[0]), len(offs) - 1
    assert total > int(offs[-1]) // 2 + 2 * n + 1024 and total > 3 * len(exp.tokens), "tokens average several ids: the first block is too small"
    v = env.words().vocabulary(vocab, 1, wordpiece=True)
    out = (np.full(total - 1, SENTINEL, dtype=np.int32), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8))
    with pytest.raises(_lib.KgpuError) as e:
        v.encode_packed(utf8, offs, out=out)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and str(total) in str(e.value) and (out[0] == SENTINEL).all()
    out = (np.full(total, SENTINEL, dtype=np.int32), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8))
    same(v.encode_packed(utf8, offs, out=out), want)
    got = C.c_uint64(0)   # a capacity of nothing: the sizing call
    rc = _lib.lib().kgpu_encode_batch(v.handle, utf8.ctypes.data, offs.ctypes.data, n, None, 0, out[1].ctypes.data, None, C.byref(got))
    assert rc == _lib.KGPU_ERR_CAPACITY and got.value == total
    same(v.encode_packed(utf8, offs), want)   # (without out=: the binding's own retry)
    same(v.encode_text("".join(s + "\n" for s in sents).encode()), want)
    v.close()


# ---- 4. a list that holds every word: the plain vocabulary's ids, byte for byte ------------------------------------------------------------------------
def test_equivalence_with_a_plain_vocabulary(env, mixed):
    utf8, offs, tokens, words, _ = mixed
    vocab = SPECIALS + sorted({w for s in words for w in s} - set(SPECIALS))
    want = E.encode_words(words, vocab, 1, 2, 3)
    assert 1 not in want[0]
    same(WP.encode_words(words, vocab, 1, 2, 3), want)   # (the reference: every word is whole)
    plain = env.words().vocabulary(vocab, 1, 2, 3)
    wp = env.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
    a, b = plain.encode_packed(utf8, offs), wp.encode_packed(utf8, offs)
    same(a, want, "the plain vocabulary runs what it ran")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert plain.info() == wp.info() and wp.wordpiece_info()["rows_split"] == 0
    from kanpyo_amd import _lib

    with pytest.raises(_lib.KgpuError) as e:
        plain.wordpiece_info()
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    plain.close(); wp.close()


# ---- 5. a mixed corpus against the reference -----------------------------------------------------------------------------------------------------------
def test_mixed_corpus(env, mixed):
    utf8, offs, tokens, words, vocab = mixed
    assert len(offs) - 1 >= 2200
    for kw in ({}, {"field": 7}):
        stats = {}
        want = ref_ids(env, utf8, offs, vocab, 1, 2, 3, tokens=tokens, kw=kw, stats=stats)
        kept = sum(stats.values())
        assert stats["whole"] > 0 and stats["unk"] > 0 and stats["split"] * 10 >= kept, stats
        v = env.words(**kw).vocabulary(vocab, 1, 2, 3, wordpiece=True)
        ids, ioff, status = v.encode_packed(utf8, offs)
        assert not status.any()
        same((ids, ioff), want, str(kw))
        rows = WP.rows(env.known, env.unk, env.nk, env.nu, ref_spec(**kw), env.keys, vocab, 1)
        wi = v.wordpiece_info()
        assert wi["rows_split"] == sum(1 for r in rows if r is not None and len(r) > 1) > 0 and wi["row_piece_ids"] == sum(len(r) for r in rows if r is not None and len(r) != 1)
        v.close()


@pytest.mark.parametrize("hooks", [{"KGPU_POOL": "0"}, {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}, {"KGPU_NO_SMALL_CALLS": "1"}])
def test_forced_chains(env, mixed, hooks, monkeypatch):
    for name, val in hooks.items():
        monkeypatch.setenv(name, val)
    e = _Env(env.dict, env.known, env.unk)   # (a fresh handle: the chain is planned per context)
    e.keys = env.keys
    utf8, offs = _packed(corpus_of(env.sd, env.keys, 200, 100, 40, 11))
    vocab = mixed[4]
    stats = {}
    want = ref_ids(e, utf8, offs, vocab, 1, None, 3, stats=stats)
    assert stats["whole"] > 0 and stats["unk"] > 0 and stats["split"] * 10 >= sum(stats.values()), stats
    v = e.words().vocabulary(vocab, 1, None, 3, wordpiece=True)
    same(v.encode_packed(utf8, offs), want)
    v.close()


# ---- 6. text, chunks, threads, lifetime -----------------------------------------------------------------------------------------------------------------
def test_text_chunks_and_the_packed_call_agree(env, mixed, monkeypatch):
    from kanpyo_amd.tokenizer import split_lines

    utf8, offs, _, _, vocab = mixed
    block = b"".join(utf8[int(offs[i]) : int(offs[i + 1])].tobytes() + [b"\r\n", "　\n".encode(), b" \t\n", b"\n"][i % 4] for i in range(len(offs) - 1))
    utf8, offs = split_lines(block)
    want = ref_ids(env, utf8, offs, vocab, 1, 2, 3)
    v = env.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
    same(v.encode_packed(utf8, offs), want, "one call")
    ids, ioff, st = v.encode_text(block)
    assert len(st) == len(offs) - 1 and not st.any()
    same((ids, ioff), want, "text")
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "1000")
    same(v.encode_packed(utf8, offs), want, "chunks")
    same(v.encode_text(block), want, "text in chunks")
    v.close()


def test_eight_threads_on_one_vocab(env, mixed):
    vocab = mixed[4]
    v = env.words().vocabulary(vocab, 1, 2, None, wordpiece=True)
    corpora, wants = [], []
    for t in range(8):
        utf8, offs = _packed(corpus_of(env.sd, env.keys, 150 + 50 * t, 100, 5, 20 + t))
        corpora.append((utf8, offs))
        wants.append(ref_ids(env, utf8, offs, vocab, 1, 2, None))
    errors = []

    def work(t):
        try:
            for _ in range(2):
                ids, ioff, st = v.encode_packed(*corpora[t])
                if st.any() or not np.array_equal(ids, wants[t][0]) or not np.array_equal(ioff, wants[t][1]):
                    errors.append(f"thread {t}: the ids differ")
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    v.close()


def test_a_vocab_outlives_its_words_handle_and_its_tokenizer(mixed):
    from kanpyo_amd import Tokenizer, synth
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    keys = synth.record_surfaces(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    info = tok.info()
    utf8, offs = _packed(corpus_of(sd, keys, 300, 100, 10, 5))
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 8)
    vocab = mixed[4]
    want = WP.encode(utf8, offs, exp.tokens, exp.offsets, known, unk, info["n_morphs"], info["n_unk_morphs"], ref_spec(), keys, vocab, 1, None, 3)
    w = tok.words()
    v = w.vocabulary(vocab, 1, None, 3, wordpiece=True)
    w.close()
    tok.close()
    same(v.encode_packed(utf8, offs), want)
    same(v.encode_packed(utf8, offs), want)
    v.close()


# ---- 7. encode_tensor -----------------------------------------------------------------------------------------------------------------------------------
def test_encode_tensor(env, mixed, tmp_path):
    import torch

    from kanpyo_amd.vocab import Vocab

    utf8, offs, tokens, _, vocab = mixed
    n = 500
    sents = [utf8[int(offs[i]) : int(offs[i + 1])].tobytes() for i in range(n)] + [b"\xff", b""]
    offs2 = np.concatenate([offs[: n + 1], [offs[n], offs[n]]]).astype(np.uint64)   # (the reference skips the invalid line: no tokens)
    toff2 = np.concatenate([tokens[1][: n + 1], [tokens[1][n], tokens[1][n]]]).astype(np.uint64)
    want = ref_ids(env, utf8, offs2, vocab, 1, 2, 3, tokens=(tokens[0], toff2))
    assert len(want[0]) > int(toff2[-1]) + 2 * (n + 2), "more ids than records and bos / eos: the first id buffer is too small"
    v = env.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
    ids, off, st = v.encode_tensor(sents)
    assert ids.is_cuda and off.is_cuda and st.is_cuda and ids.dtype == torch.int32 and off.dtype == torch.int64 and st.dtype == torch.uint8
    assert st.cpu().tolist() == [0] * n + [1, 0]
    same((ids.cpu().numpy(), off.cpu().numpy().astype(np.uint64)), want)
    for width in (5, 16, 64):
        pids, lengths, st = v.encode_tensor(sents, width=width, pad_id=-1)
        assert pids.is_cuda and pids.dtype == torch.int32 and tuple(pids.shape) == (n + 2, width) and lengths.dtype == torch.int64
        assert np.array_equal(pids.cpu().numpy(), WP.padded(want[0], want[1], width, -1, 3))
        assert np.array_equal(lengths.cpu().numpy(), np.minimum(np.diff(want[1].astype(np.int64)), width))
    # the file form: a vocab.txt as it is
    path = tmp_path / "vocab.txt"
    v.save(path)
    v2 = Vocab.load(env.words(), path, unk="[UNK]", bos="[CLS]", eos="[SEP]", wordpiece=True)
    assert v2.words == v.words and (v2.unk_id, v2.bos_id, v2.eos_id, v2.wordpiece) == (1, 2, 3, True)
    same(v2.encode_packed(utf8, offs2), want)
    v.close(); v2.close()


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------------------------------
def test_cli_wordpiece(env, mixed, tmp_path):
    from kanpyo_amd.dictfile import DictFile, save_dict
    from kanpyo_amd.tokenizer import split_lines

    path = tmp_path / "t.dict"
    save_dict(DictFile(env.sd.dict, env.known, env.unk), str(path))
    sents = corpus_of(env.sd, env.keys, 300, 200, 0, 13)
    data = "".join(s + ["\r\n", "　\n", " \t\n", "\n"][i % 4] for i, s in enumerate(sents)).encode()
    vocab = [w for w in mixed[4] if b"\n" not in w]
    vfile = tmp_path / "vocab.txt"
    vfile.write_bytes(b"".join(w + b"\n" for w in vocab))
    text = lambda want: b"".join(" ".join(map(str, want[0][int(want[1][i]) : int(want[1][i + 1])].tolist())).encode() + b"\n" for i in range(len(want[1]) - 1))   # noqa: E731
    pieces = ref_ids(env, *split_lines(data), vocab, 1, 2, 3)
    plain = E.encode_words(E.sentence_words(*split_lines(data), *_oracle(env, data), env.known, env.unk, env.nk, env.nu, ref_spec(), env.keys), vocab, 1, 2, 3)
    assert len(pieces[0]) > len(plain[0])
    at_prefix = [b"@" + w[2:] if w.startswith(b"##") else w for w in vocab]
    envv = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "encode", "-c", str(path), "--unk", "[UNK]", "--bos", "[CLS]", "--eos", "[SEP]"]
    run = lambda extra: subprocess.run(cmd + extra, input=data, capture_output=True, env=envv, cwd=ROOT, timeout=600)   # noqa: E731
    r = run(["--vocab", str(vfile), "--wordpiece", "--block-bytes", "20000", "--split", "device"])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == text(pieces)
    r = run(["--vocab", str(vfile)])
    assert r.returncode == 0 and r.stdout == text(plain), "without --wordpiece: the plain ids"
    afile = tmp_path / "vocab_at.txt"
    afile.write_bytes(b"".join(w + b"\n" for w in at_prefix))
    r = run(["--vocab", str(afile), "--wordpiece", "--prefix", "@", "--max-word-chars", "3"])
    assert r.returncode == 0 and r.stdout == text(ref_ids(env, *split_lines(data), at_prefix, 1, 2, 3, prefix=b"@", max_chars=3))
    r = run(["--vocab", str(vfile), "--prefix", "@"])
    assert r.returncode == 2 and r.stdout == b"" and "--wordpiece" in r.stderr.decode()
    r = run(["--vocab", str(vfile), "--wordpiece", "--prefix", "123456789"])
    assert r.returncode == 2 and r.stdout == b""


def _oracle(env, data):
    from kanpyo_amd.tokenizer import split_lines

    exp = env.orc.tokenize_batch(*split_lines(data), 8)
    return exp.tokens, exp.offsets
