"""The word counts on the device (include/kanpyo_gpu.h, "word counts"; kgpu_count.hip): kgpu_count_batch, kgpu_count_text,
kgpu_count_words_device, the read-out, the C consumer and `python -m kanpyo_amd count`.  Expected values always come from the oracle's tokens
(or crafted records) through tests/count_ref.py -- never from the library.  No tolerance: every read-out is compared entry for entry, in order."""
import os
import subprocess
import sys
import threading
from collections import Counter

import numpy as np
import pytest

import count_ref as CR
import lines_ref as R
import words_ref as W
from conftest import ROOT, load_golden
from record_cases import (LENGTHS, POS_DROP, SMALL_KEYS, SPECS, _Dev, _Env, _fixture_env, _write_dict_dir, crafted_want, dev_count, env, holds, mixed, ref_spec, small_ctx,  # noqa: F401
                          small_env)   # (env, mixed, small_ctx, small_env: the fixtures)

pytestmark = pytest.mark.gpu

SMALL = {"table_slots": 1 << 14, "key_bytes": 1 << 20}   # most handles here: a default one holds 320 MiB of device memory


def expect(env, utf8, offs, kw, keys, tokens=None, into=None, ids=None):
    """The reference's Counter for a batch: the oracle's tokens (own records: every key is asserted to be the text's bytes) or the given ones."""
    exp = env.orc.tokenize_batch(utf8, offs, 8) if tokens is None else None
    t, to = (exp.tokens, exp.offsets) if tokens is None else tokens
    return CR.count(utf8, offs, t, to, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), keys, own_records=tokens is None, into=into, ids=ids)


def mixed_want(env, mixed, kw, ids=None):
    utf8, offs, tokens = mixed
    return CR.count(utf8, offs, *tokens, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), env.keys, own_records=True, ids=ids)


# ---- 1. the fixture golden -------------------------------------------------------------------------------------------------------------------
def test_fixture_golden_host_form_and_c_consumer(tmp_path):
    from kanpyo_amd import _lib
    from kanpyo_amd.dictfile import DictFile

    e = _fixture_env()
    cases = load_golden("fixture_counts.json")["cases"]
    exe = str(tmp_path / "counts_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "counts_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    blobs = _write_dict_dir(e.dict, DictFile(e.dict, e.known, e.unk), tmp_path)
    for c in cases:
        kw = {"field": None if c["field"] < 0 else c["field"], "drop": tuple(c["names"]) if c["filter"] == 1 else (), "keep": tuple(c["names"]) if c["filter"] == 2 else ()}
        want = [(w.encode(), n) for w, n in c["counts"]]
        # (filter 1 / 2 with an empty list: Tokenizer.words cannot say it -- the C consumer below does)
        if not (c["filter"] and not c["names"]):
            k = e.words(**kw).counter(**SMALL)
            st = k.add(c["sentences"])
            assert not st.any() and k.most_common() == want, c
            assert k.info()["sentences"] == len(c["sentences"])
            k.close()
        data = "".join(s + "\n" for s in c["sentences"]).encode()
        for top in (0, 2):
            r = subprocess.run([exe, str(blobs), str(c["field"]), str(c["filter"]), str(top), *c["names"]], input=data, capture_output=True, timeout=300)
            assert r.returncode == 0, r.stderr.decode()
            assert r.stdout == b"".join(b"%d\t%s\n" % (n, w) for w, n in (want[:top] if top else want)), (c, top)
    r = subprocess.run([exe, str(blobs), "-1", "0", "0"], input="テスト\n".encode() + b"\xff\n" + "辞書\n".encode(), capture_output=True, timeout=300)
    assert r.returncode == 101 and r.stdout == b""


# ---- 2. a mixed corpus under every spec -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPECS))
def test_mixed_corpus(env, mixed, name):
    utf8, offs, (tokens, toff) = mixed
    kw = SPECS[name]
    ids, wc = {}, {}
    want = mixed_want(env, mixed, kw, ids)
    # the case is not trivial, by the reference alone
    W.render(utf8, offs, tokens, toff, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), wc)
    assert sum(want.values()) == wc["tokens"] - wc["dropped"] > 0
    if name != "keep":   # (KEEP [感動詞] keeps a few hundred tokens of which no two ids share a word)
        assert any(len(v) > 1 for v in ids.values()), "no word merges two ids"
    if name in ("drop", "keep"):
        assert 0 < wc["dropped"] < wc["tokens"], "the filter must drop some tokens and keep some"
    raw = utf8.tobytes()
    sent = np.repeat(np.arange(len(offs) - 1), np.diff(toff.astype(np.int64)))
    unk_at = np.flatnonzero(tokens["cls"] == W.UNKNOWN)
    surf = Counter(raw[int(offs[sent[i]]) + int(tokens["position"][i]) : int(offs[sent[i]]) + int(tokens["position"][i]) + int(tokens["byte_len"][i])] for i in unk_at)
    assert max(surf.values()) >= 2 and len(surf) > 100, "no unknown-class surface occurs twice"
    k = env.words(**kw).counter(**SMALL)
    st = k.add_packed(utf8, offs)
    assert not st.any()
    info = holds(k, want)
    assert info["sentences"] == len(offs) - 1
    if name in ("surface", "field40"):   # every unknown surface has one slot and a key of its own, nothing else is in the table
        assert info["table_slots_used"] == len(surf) and info["key_bytes_used"] >= 16 * len(surf)
    k.close()


# ---- 3. key shapes: crafted records through the device form ------------------------------------------------------------------------------------
U, K = R.UNKNOWN, R.KNOWN


def test_key_shapes(small_env, small_ctx):
    rng = np.random.default_rng(11)
    body = rng.integers(1, 256, size=4000, dtype=np.uint8).tobytes()
    # every length, twice each at different positions (the second copy placed behind the first: equal bytes at another address)
    s_len = b"".join(body[:L] + b"|" + body[:L] for L in LENGTHS)
    recs_len, at = [], 0
    for L in LENGTHS:
        recs_len += [(1, U, at, L), (2, U, at + L + 1, L), (0, K, at, L)]
        at += 2 * L + 1
    # the same 37 bytes at every source alignment 0..15 of a sentence that starts 16-byte aligned: one entry of 16
    word = body[100:137]
    s_align, recs_align, at = b"", [], 0
    for a in range(16):
        pad = (a - len(s_align)) % 16
        s_align += b"\0" * pad + word
        recs_align.append((1, U, len(s_align) - len(word), len(word)))
    # keys that differ in their last byte only; a key and its proper prefix; "a" against "a\0"; a 3072-byte pair differing at the end
    big = body[200:3272]
    s_near = b"abcdefgXabcdefgYa\0" + big[:-1] + b"\x01" + big[:-1] + b"\x02"
    recs_near = [(1, U, 0, 8), (1, U, 8, 8), (1, U, 8, 8), (2, U, 0, 7), (1, U, 16, 1), (1, U, 16, 2), (1, U, 16, 2), (0, U, 17, 1),
                 (1, U, 18, 3072), (1, U, 18 + 3072, 3072), (1, U, 18 + 3072, 3072), (1, U, 18, 3071)]
    # a known record whose bytes are not its key; dummies with noise; a key that ends at the last byte of the last sentence of the buffer
    s_known = b"xyz"
    recs_known = [(1, K, 0, 3), (1, K, 1, 0), (2, K, 0, 1), (3, K, 3, 0), (7, R.DUMMY, 99, 99), (0, R.DUMMY, 0, 0)]
    s_last = b"....tail"
    recs_last = [(1, U, 4, 4), (1, U, 4, 4), (2, U, 8, 0)]
    lead = b"\0" * 16   # (sentence 1 starts 16-byte aligned)
    case = R.pack([lead, s_align, s_len, s_near, b"", s_known, s_last], [[], recs_align, recs_len, recs_near, [], recs_known, recs_last])
    assert int(case[1][1]) % 16 == 0 and int(case[1][-1]) == len(case[0])
    want = crafted_want(small_env, case, {})
    assert want[word] == 16 and want[b""] == 4 and want[b"a"] == 1 and want[b"a\0"] == 2 and want[b"\0"] == 1 and want[b"tail"] == 2
    assert want["テスト".encode()] == 2 and want["辞書".encode()] == 1 and want["形態素".encode()] == 1 and b"xyz" not in want
    assert want[big[:-1] + b"\x01"] == 1 and want[big[:-1] + b"\x02"] == 2 and want[big[:-1]] == 1
    k = small_env.words().counter(table_slots=256, key_bytes=1 << 16)
    assert dev_count(small_ctx, k, case) == (0, sum(want.values()))
    holds(k, want)
    # a pool name and a surface with equal bytes are one entry: field 0 makes "未知" the word of every unknown record with an id
    name = "未知".encode()
    case2 = R.pack([name + b"--" + name], [[(1, U, 0, 3), (2, U, 2, 1), (0, U, 0, 6), (0, K, 8, 6), (0, U, 6, 2)]])
    want2 = crafted_want(small_env, case2, {"field": 0})
    assert want2 == Counter({name: 4, b"--": 1})
    k2 = small_env.words(field=0).counter(table_slots=64, key_bytes=4096)
    assert dev_count(small_ctx, k2, case2) == (0, 5)
    holds(k2, want2)
    k.close(); k2.close()


def test_repeated_character_through_the_tokenizer():
    """The fixture dictionary groups hiragana into one unknown word: "あ" * k is one surface of 3 k bytes up to the 1024-character limit of an
    unknown word (lattice.rs:55); the oracle cuts "あ" * 1025 into the 1024-character word and a single "あ", so the words are "あ" * 1, 2 and 1024."""
    e = _fixture_env()
    from kanpyo_amd.tokenizer import pack_sentences

    sents = ["あ" * k for k in (1, 2, 1024, 1025)] * 2 + ["あ" * 1024]
    utf8, offs = pack_sentences(sents)
    want = expect(e, utf8, offs, {}, SMALL_KEYS)
    assert want[("あ" * 1024).encode()] >= 3 and len(want) >= 3 and sum(want.values()) >= len(sents) and max(len(w) for w in want) == 3072
    k = e.words().counter(table_slots=64, key_bytes=1 << 16)
    assert not k.add_packed(utf8, offs).any()
    holds(k, want)
    k.close()


# ---- 4. small tables ---------------------------------------------------------------------------------------------------------------------------
def _distinct_case(n_words, per_word=2, width=6):
    """One sentence per word: n_words distinct unknown surfaces of `width` bytes, each counted per_word times."""
    sents = [b"%0*d" % (width, (7919 * i) % 10**width) for i in range(n_words)]   # (7919 is coprime to 10: distinct below 10^width words)
    return R.pack(sents, [[(1, U, 0, width)] * per_word for _ in sents])


def _rowdet_case():
    return R.pack([b"abcdef"] * 50, [[(1, K, 0, 3), (2, K, 3, 3), (3, K, 0, 6), (1, K, 2, 2)]] * 50)


def test_small_table_wraps_and_overflows(small_env, small_ctx):
    from kanpyo_amd import _lib

    w = small_env.words()
    k = w.counter(table_slots=64, key_bytes=1 << 16)
    assert k.info()["table_slots"] == 64
    case = _distinct_case(60)
    want = crafted_want(small_env, case, {})
    assert len(want) == 60
    assert dev_count(small_ctx, k, case) == (0, 120)
    info = holds(k, want)
    assert info["table_slots_used"] == 60
    k.reset()
    # 200 distinct words: 64 fit
    case = _distinct_case(200)
    want = crafted_want(small_env, case, {})
    assert len(want) == 200
    rc, counted = dev_count(small_ctx, k, case)
    assert rc == _lib.KGPU_ERR_CAPACITY
    info = k.info()
    got = k.most_common()
    assert info["table_slots_used"] == 64 and len(got) == 64
    assert all(n <= want[wd] for wd, n in got)                                        # every reported count <= the true count
    assert sum(n for _, n in got) + info["overflow_tokens"] == sum(want.values())     # reported + overflow = tokens kept
    assert info["tokens_counted"] == counted == sum(n for _, n in got) and info["overflow_tokens"] > 0
    assert got == CR.ordered(Counter(dict(got)))                                      # ... and still in rule 5's order
    # the handle then counts a batch of row-determined words exactly
    before = Counter(dict(got))
    case = _rowdet_case()
    assert dev_count(small_ctx, k, case) == (0, 200)
    after = Counter(dict(k.most_common()))
    assert after - before == crafted_want(small_env, case, {}) and k.info()["overflow_tokens"] == info["overflow_tokens"]
    k.close()


def test_key_arena_too_small_for_one_key(small_env, small_ctx):
    from kanpyo_amd import _lib

    k = small_env.words().counter(table_slots=64, key_bytes=2048)
    text = bytes(range(1, 256)) * 13
    case = R.pack([text[:3100]], [[(1, U, 0, 3072), (1, U, 10, 5), (1, U, 0, 3072), (2, K, 0, 1)]])
    want = crafted_want(small_env, case, {})
    rc, counted = dev_count(small_ctx, k, case)
    assert rc == _lib.KGPU_ERR_CAPACITY and counted == 2
    info = k.info()
    got = k.most_common()
    assert info["overflow_tokens"] == 2 and info["key_bytes"] == 2048 and info["key_bytes_used"] <= 2048
    assert sorted(got) == sorted([(text[10:15], 1), ("辞書".encode(), 1)])
    assert sum(n for _, n in got) + info["overflow_tokens"] == sum(want.values())
    assert dev_count(small_ctx, k, _rowdet_case()) == (0, 200)
    assert Counter(dict(k.most_common())) - Counter(dict(got)) == crafted_want(small_env, _rowdet_case(), {})
    k.close()


# ---- 5. simultaneous first insertion -----------------------------------------------------------------------------------------------------------
def test_simultaneous_first_insertion(small_env, small_ctx):
    many = R.pack([b"brand-new-word"] * 4096, [[(1, U, 0, 14)]] * 4096)
    one = R.pack([b"0123456789"], [[(2, U, 3, 5)] * 200])
    outs = []
    for _ in range(2):
        k = small_env.words().counter(table_slots=64, key_bytes=1 << 20)
        assert dev_count(small_ctx, k, many) == (0, 4096)
        assert dev_count(small_ctx, k, one) == (0, 200)
        holds(k, Counter({b"brand-new-word": 4096, b"34567": 200}))
        assert k.info()["table_slots_used"] == 2
        outs.append(k.most_common())
        k.close()
    assert outs[0] == outs[1]


# ---- 6. a hot key ------------------------------------------------------------------------------------------------------------------------------
def test_hot_key(env):
    from kanpyo_amd.tokenizer import pack_sentences

    word = env.keys[len(env.keys) // 2]
    utf8, offs = pack_sentences([word * 32] * 4096)
    want = expect(env, utf8, offs, {}, env.keys)   # whatever the oracle segments
    assert sum(want.values()) >= 4096 * 8
    for name in ("surface", "field7"):
        k = env.words(**SPECS[name]).counter(**SMALL)
        assert not k.add_packed(utf8, offs).any()
        holds(k, want if name == "surface" else expect(env, utf8, offs, SPECS[name], env.keys))
        k.close()


# ---- 7. accumulation ---------------------------------------------------------------------------------------------------------------------------
def test_one_call_chunks_and_text_agree(env, mixed, monkeypatch):
    from kanpyo_amd.tokenizer import split_lines

    utf8, offs, _ = mixed
    kw = SPECS["drop"]
    block = b"".join(utf8[int(offs[i]) : int(offs[i + 1])].tobytes() + [b"\r\n", "　\n".encode(), b" \t\n", b"\n"][i % 4] for i in range(len(offs) - 1))
    utf8, offs = split_lines(block)   # (the corpus as read_line + trim_end leave it)
    assert len(offs) - 1 >= 2200
    want = expect(env, utf8, offs, kw, env.keys)
    k = env.words(**kw).counter(**SMALL)
    k.add_packed(utf8, offs)
    holds(k, want)
    one = k.most_common()
    k.add_packed(utf8, offs)   # adding twice doubles every count
    holds(k, Counter({w: 2 * n for w, n in want.items()}))
    k.reset()
    assert k.most_common() == [] and k.info()["tokens_counted"] == 0 and k.info()["sentences"] == 0 and k.info()["table_slots_used"] == 0
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "1000")
    k.add_packed(utf8, offs)
    assert k.most_common() == one
    k.reset()
    st = k.add_text(block)
    assert len(st) == len(offs) - 1 and not st.any() and k.most_common() == one
    monkeypatch.delenv("KGPU_HOST_CHUNK_SENTS")
    k.reset()
    k.add_text(block)
    assert k.most_common() == one and k.info()["sentences"] == len(offs) - 1
    k.close()


@pytest.mark.parametrize("hooks", [{"KGPU_POOL": "0"}, {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}, {"KGPU_NO_SMALL_CALLS": "1"}])
def test_forced_chains(env, hooks, monkeypatch):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    for name, v in hooks.items():
        monkeypatch.setenv(name, v)
    e = _Env(env.dict, env.known, env.unk)   # (a fresh handle: the chain is planned per context)
    utf8, offs = pack_sentences(synth.make_corpus(env.sd, 300, 3, "cfg2") + synth.make_corpus(env.sd, 40, 4, "cfg3"))
    for name in ("surface", "field7", "drop"):
        k = e.words(**SPECS[name]).counter(**SMALL)
        k.add_packed(utf8, offs)
        holds(k, expect(e, utf8, offs, SPECS[name], env.keys))
        k.close()


@pytest.mark.parametrize("entry", ["packed", "text"])
def test_chain_rerun_counts_every_token_once(entry):
    """The recipe of tests/test_gpu_lines.py::test_chain_runs_again_behind_the_render: 14 clean short batches disarm the chain's tail, then a mixed
    block needs it -- the tail runs inside kgpu_ctx_sync.  The count is enqueued behind that, once."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import split_lines

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    keys = synth.record_surfaces(sd)
    k = e.words().counter(**SMALL)
    add = (lambda b: k.add_packed(*split_lines(b))) if entry == "packed" else k.add_text
    short = [s[:30].replace("\n", "") for s in synth.make_corpus(sd, 600, 9, "cfg2")]
    clean = "".join(s + "\n" for s in short).encode()
    for _ in range(14):
        add(clean)
    assert e.tok.routing()["tail_reruns"] == 0
    k.reset()
    mixed_sents = short[:100] + ["ア" * 900, "漢字かな" * 150] + [s.replace("\n", "") for s in synth.make_corpus(sd, 5, 10, "cfg3")] + short[100:200]
    block = "".join(s + "\n" for s in mixed_sents).encode()
    st = add(block)
    reruns = e.tok.routing()["tail_reruns"]
    print(f"{entry}: tail_reruns {reruns}")
    assert reruns >= 1, "the mixed batch did not take the tail pass"
    assert not st.any()
    holds(k, expect(e, *split_lines(block), {}, keys))
    k.close()


# ---- 8. threads and lifetimes ------------------------------------------------------------------------------------------------------------------
def test_eight_threads_add_into_one_handle(env):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    kw = SPECS["field7"]
    k = env.words(**kw).counter(**SMALL)
    corpora, want = [], Counter()
    for t in range(8):
        utf8, offs = pack_sentences(synth.make_corpus(env.sd, 300 + 100 * t, 20 + t, "cfg2") + synth.make_corpus(env.sd, 5, 40 + t, "cfg3"))
        corpora.append((utf8, offs))
        expect(env, utf8, offs, kw, env.keys, into=want)
    errors = []

    def work(t):
        try:
            if k.add_packed(*corpora[t]).any():
                errors.append(f"thread {t}: a status byte is set")
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    info = holds(k, want)
    assert info["sentences"] == sum(len(o) - 1 for _, o in corpora)
    k.close()


def test_a_handle_outlives_its_words_handle_and_its_tokenizer():
    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    info = tok.info()
    w = tok.words(field=7, drop=POS_DROP)
    k = w.counter(**SMALL)
    utf8, offs = pack_sentences(synth.make_corpus(sd, 500, 3, "cfg2"))
    k.add_packed(utf8, offs)
    w.close()
    tok.close()
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 8)
    want = CR.count(utf8, offs, exp.tokens, exp.offsets, known, unk, info["n_morphs"], info["n_unk_morphs"], ref_spec(field=7, drop=POS_DROP),
                    synth.record_surfaces(sd), own_records=True)
    k.add_packed(utf8, offs)
    holds(k, Counter({wd: 2 * n for wd, n in want.items()}))
    k.close()


# ---- 9. status bytes and empty input -----------------------------------------------------------------------------------------------------------
def test_invalid_utf8_neighbours_and_empty_input(env):
    from kanpyo_amd.tokenizer import pack_sentences

    word = env.keys[7]
    utf8, offs = pack_sentences([b"\xe3\x81", word.encode(), b"\xff", b"", word.encode(), b"\xf8\x88\x80\x80\x80"])
    valid = pack_sentences([word, "", word])
    for name in ("surface", "field7", "drop"):
        k = env.words(**SPECS[name]).counter(**SMALL)
        assert k.add_packed(utf8, offs).tolist() == [1, 0, 1, 0, 0, 1], name
        holds(k, expect(env, *valid, SPECS[name], env.keys))
        assert k.info()["sentences"] == 6
        assert k.add([]).tolist() == [] and k.add([""]).tolist() == [0] and k.add_text(b"").tolist() == [] and k.add_text(b"\n\n").tolist() == [0, 0]
        holds(k, expect(env, *valid, SPECS[name], env.keys))
        k.close()
    k = env.words().counter(**SMALL)
    assert k.most_common() == [] and k.most_common(5) == [] and k.most_common(0) == []
    k.close()


# ---- 10. bad records, foreign contexts ---------------------------------------------------------------------------------------------------------
def test_one_bad_record_and_a_foreign_context(small_env, small_ctx):
    from kanpyo_amd import _lib
    from kanpyo_amd.device import DeviceContext

    rng = np.random.default_rng(7)
    case = R.many_case(rng, 1025, small_env.nk, small_env.nu, long_at=(3, 700))
    utf8, offsets, tokens, tok_offsets = case
    want = crafted_want(small_env, case, {})
    k = small_env.words().counter(table_slots=1 << 12, key_bytes=1 << 18)
    s, kk = 700, 150
    B = int(offsets[s + 1] - offsets[s])
    r = int(tok_offsets[s]) + kk
    for field, value in (("id", small_env.nk + 1), ("id", -1), ("cls", 3), ("position", B + 1), ("byte_len", B + 1)):
        bad = tokens.copy()
        bad[r] = (1, R.KNOWN, 0, 0, 0, 0)
        bad[r][field] = value
        with pytest.raises(ValueError):
            crafted_want(small_env, (utf8, offsets, bad, tok_offsets), {})
        rc, _ = dev_count(small_ctx, k, (utf8, offsets, bad, tok_offsets))
        assert rc == _lib.KGPU_ERR_INVALID_ARG, (field, value)
        k.reset()
    back = tok_offsets.copy()
    back[20] = back[19] - 2
    assert dev_count(small_ctx, k, (utf8, offsets, tokens, back))[0] == _lib.KGPU_ERR_INVALID_ARG
    k.reset()
    assert dev_count(small_ctx, k, case) == (0, sum(want.values()))   # after the reset: exact again
    holds(k, want)
    # a context of another dictionary
    other = _Env(small_env.dict, small_env.known, small_env.unk)
    ctx = DeviceContext(other.tok)
    d = _Dev(case)
    with pytest.raises(_lib.KgpuError) as e:
        ctx.count_words(k, d.utf8.data_ptr(), d.off.data_ptr(), d.n, d.tok.data_ptr(), d.toff.data_ptr())
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    ctx.close()
    holds(k, want)
    k.close()


# ---- 11. the CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli(env, tmp_path):
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile, save_dict
    from kanpyo_amd.tokenizer import pack_sentences, split_lines

    path = tmp_path / "t.dict"
    save_dict(DictFile(env.sd.dict, env.known, env.unk), str(path))
    sents = synth.make_corpus(env.sd, 1200, 11, "cfg2")
    raw = [s + ["\r\n", "　\n", " \t\n", "\n"][i % 4] for i, s in enumerate(sents)]
    raw.insert(5, "\n")
    data = "".join(raw).encode() + "最後の行".encode()
    kw = {"field": 7, "drop": POS_DROP}
    want = expect(env, *split_lines(data), kw, env.keys)
    lines = lambda top=None: b"".join(b"%d\t%s\n" % (n, w) for w, n in CR.ordered(want, top))   # noqa: E731
    envv = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "count", "-c", str(path), "--reading", "--drop", ",".join(POS_DROP)]
    run = lambda extra, inp=data: subprocess.run(cmd + extra, input=inp, capture_output=True, env=envv, cwd=ROOT, timeout=600)   # noqa: E731
    for split in ("host", "device"):   # stdin in small blocks, split on the host and on the device
        r = run(["--block-bytes", "20000", "--split", split])
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == lines(), split
    r = run(["--top", "10"])
    assert r.returncode == 0 and r.stdout == lines(10) and r.stdout.count(b"\n") == 10
    # an invalid line: status 101, its number on stderr, nothing on stdout
    cut = data.index(b"\n", len(data) // 2) + 1
    broken = data[:cut] + b"\xff\xfe\n" + data[cut:]
    bad_line = data[:cut].count(b"\n") + 1
    r = run(["--block-bytes", "20000"], broken)
    assert r.returncode == 101 and r.stdout == b"" and f"line {bad_line}:" in r.stderr.decode()
    r = run(["--block-bytes", "20000", "--skip-invalid", "--split", "device"], broken)
    assert r.returncode == 0 and r.stdout == lines() and f"line {bad_line}:" in r.stderr.decode()
    # INPUT argument: that one string, untrimmed
    one = sents[0] + " "
    want1 = expect(env, *pack_sentences([one]), {}, env.keys)
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "count", "-c", str(path), one], capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout == b"".join(b"%d\t%s\n" % (n, w) for w, n in CR.ordered(want1))
