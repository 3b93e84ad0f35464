"""The vocabulary ids on the device (include/kanpyo_gpu.h, "vocabulary ids"; kgpu_encode.hip): kgpu_encode_batch, kgpu_encode_text,
kgpu_encode_device ragged and padded, Vocab.encode_tensor, the C consumer and `python -m kanpyo_amd encode`.  Expected values always come from
the oracle's tokens (or crafted records) through tests/encode_ref.py -- never from the library.  No tolerance: ids and all n + 1 offsets are
compared exactly."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import count_ref as CR
import encode_ref as E
import lines_ref as R
import words_ref as W
from conftest import ROOT, load_golden
from record_cases import (LENGTHS, POS_DROP, SENTINEL, SMALL_KEYS, SPECS, _Dev, _Env, _fixture_env, _write_dict_dir, check_ragged, crafted_ids, dev_encode, env, mixed,  # noqa: F401
                          ref_spec, same, small_ctx, small_env)   # (env, mixed, small_ctx, small_env: the fixtures)

pytestmark = pytest.mark.gpu

U, K = R.UNKNOWN, R.KNOWN


def ref_ids(env, utf8, offs, kw, keys, vocab, unk, bos=None, eos=None, tokens=None, sources=None):
    """The reference's (ids, id_offsets) for a batch: the oracle's tokens, or the given (tokens, tok_offsets)."""
    if tokens is None:
        exp = env.orc.tokenize_batch(utf8, offs, 8)
        tokens = (exp.tokens, exp.offsets)
    words = E.sentence_words(utf8, offs, *tokens, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), keys, sources)
    return E.encode_words(words, vocab, unk, bos, eos)


_TOP_HALF = {}


def top_half(env, mixed, kw):
    """The vocabulary of most tests here: <pad>, <unk>, then the top half of the reference's own counts of the mixed corpus (computed once per spec)."""
    key = repr(sorted(kw.items()))
    if key not in _TOP_HALF:
        utf8, offs, tokens = mixed
        counts = CR.count(utf8, offs, *tokens, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), env.keys, own_records=True)
        order = [w for w, _ in CR.ordered(counts)]
        _TOP_HALF[key] = ([b"<pad>", b"<unk>"] + order[: (len(order) + 1) // 2], counts)
    vocab, counts = _TOP_HALF[key]
    return list(vocab), counts


# ---- 1. the fixture golden -------------------------------------------------------------------------------------------------------------------
def test_fixture_golden_host_form_and_c_consumer(tmp_path):
    from kanpyo_amd import _lib
    from kanpyo_amd.dictfile import DictFile

    e = _fixture_env()
    cases = load_golden("fixture_encode.json")["cases"]
    exe = str(tmp_path / "encode_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "encode_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    blobs = _write_dict_dir(e.dict, DictFile(e.dict, e.known, e.unk), tmp_path)
    for k, c in enumerate(cases):
        kw = {"field": None if c["field"] < 0 else c["field"], "drop": tuple(c["names"]) if c["filter"] == 1 else (), "keep": tuple(c["names"]) if c["filter"] == 2 else ()}
        v = e.words(**kw).vocabulary(c["vocab"], c["unk_id"], c["bos_id"], c["eos_id"])
        got = v.encode(c["sentences"])
        assert [g.tolist() for g in got] == c["ids"], c
        assert all(g.dtype == np.int32 for g in got) and v.info()["n_words"] == len(c["vocab"]) and v.info()["table_slots"] == 16
        v.close()
        vf = tmp_path / f"vocab{k}.txt"
        vf.write_bytes(b"".join(w.encode() + b"\n" for w in c["vocab"]))
        data = "".join(s + "\n" for s in c["sentences"]).encode()
        opt = lambda x: "-" if x is None else str(x)   # noqa: E731
        r = subprocess.run([exe, str(blobs), str(c["field"]), str(c["filter"]), str(vf), str(c["unk_id"]), opt(c["bos_id"]), opt(c["eos_id"]), *c["names"]],
                           input=data, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == b"".join(" ".join(map(str, row)).encode() + b"\n" for row in c["ids"]), c
    r = subprocess.run([exe, str(blobs), "-1", "0", str(vf), "0", "-", "-"], input="テスト\n".encode() + b"\xff\n" + "辞書\n".encode(), capture_output=True, timeout=300)
    assert r.returncode == 101 and r.stdout == b""


# ---- 2. a mixed corpus under every spec -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPECS))
def test_mixed_corpus(env, mixed, name):
    utf8, offs, tokens = mixed
    kw = SPECS[name]
    vocab, counts = top_half(env, mixed, kw)
    listed = set(vocab)
    sources = {}
    want = ref_ids(env, utf8, offs, kw, env.keys, vocab, 1, tokens=tokens, sources=sources)
    # the case is not trivial, by the reference alone
    n_unk = int((want[0] == 1).sum())
    assert 0 < n_unk < len(want[0]) == sum(counts.values()), "some kept tokens must be in the list and some must be <unk>"
    spec = ref_spec(**kw)
    unk_surface = {w for w, src in sources.items() if any(c == W.UNKNOWN and (t == 0 or W.row_word(env.unk.features(t), spec) is None) for c, t in src)}
    if name != "field0":
        assert unk_surface & listed and unk_surface - listed, "some unknown-class surface must be in the list and some must not"
    else:   # field 0 names every unknown row, and the tokenizer writes no record without a row: no unknown-class token's word is its surface
        assert not unk_surface and all(W.row_word(env.unk.features(t), spec) is not None for t in range(1, env.nu + 1))
    if name != "keep":
        assert any(len(src) > 1 for src in sources.values()), "no word is reached through two different (class, id) pairs"
    else:   # KEEP [感動詞] keeps a few hundred tokens of which no two ids share a word: every word has one source
        assert 0 < len(want[0]) < 1000 and all(len(src) == 1 for src in sources.values())
    v = env.words(**kw).vocabulary(vocab, 1)
    ids, ioff, status = v.encode_packed(utf8, offs)
    assert not status.any()
    same((ids, ioff), want, name)
    info = v.info()
    rows = E.row_ids(env.known, env.unk, env.nk, env.nu, spec, env.keys, vocab, 1)
    assert info["n_words"] == len(vocab) and info["rows_resolved"] == sum(1 for r in rows if r is not None and r != 1)
    v.close()


# ---- 3. key shapes: crafted records through the device form ------------------------------------------------------------------------------------
def half_listed(words):
    """Half of the distinct words listed, the other half absent -- and every absent word with a listed neighbour one byte or one length away."""
    words = sorted(set(words))
    listed, absent = set(words[0::2]), set(words[1::2])
    for w in sorted(absent):
        cands = [w + b"\0"] + ([w[:-1] + bytes([w[-1] ^ 1]), w[:-1]] if w else [])
        near = next(c for c in cands if c not in absent)
        listed.add(near)
    for w in absent:   # by construction, checked all the same
        assert any((len(x) == len(w) and sum(a != b for a, b in zip(x, w)) == 1) or (abs(len(x) - len(w)) == 1 and (x.startswith(w) or w.startswith(x))) for x in listed), w
    return sorted(listed), absent


def key_shapes_case():
    """tests/test_gpu_count.py::test_key_shapes' crafted batch, shape for shape."""
    rng = np.random.default_rng(11)
    body = rng.integers(1, 256, size=4000, dtype=np.uint8).tobytes()
    s_len = b"".join(body[:L] + b"|" + body[:L] for L in LENGTHS)   # every length, twice each at different positions
    recs_len, at = [], 0
    for L in LENGTHS:
        recs_len += [(1, U, at, L), (2, U, at + L + 1, L), (0, K, at, L)]
        at += 2 * L + 1
    word = body[100:137]   # the same 37 bytes at every source alignment 0..15 of a sentence that starts 16-byte aligned
    s_align, recs_align = b"", []
    for a in range(16):
        pad = (a - len(s_align)) % 16
        s_align += b"\0" * pad + word
        recs_align.append((1, U, len(s_align) - len(word), len(word)))
    big = body[200:3272]   # keys that differ in their last byte only; a key and its proper prefix; "a" against "a\0"; the 3072-byte pair
    s_near = b"abcdefgXabcdefgYa\0" + big[:-1] + b"\x01" + big[:-1] + b"\x02"
    recs_near = [(1, U, 0, 8), (1, U, 8, 8), (1, U, 8, 8), (2, U, 0, 7), (1, U, 16, 1), (1, U, 16, 2), (1, U, 16, 2), (0, U, 17, 1),
                 (1, U, 18, 3072), (1, U, 18 + 3072, 3072), (1, U, 18 + 3072, 3072), (1, U, 18, 3071)]
    s_known = b"xyz"       # a known record whose bytes are not its key; dummies with noise
    recs_known = [(1, K, 0, 3), (1, K, 1, 0), (2, K, 0, 1), (3, K, 3, 0), (7, R.DUMMY, 99, 99), (0, R.DUMMY, 0, 0)]
    s_last = b"....tail"   # a key that ends at the last byte of the buffer: no spare byte behind the text (_Dev)
    recs_last = [(1, U, 4, 4), (1, U, 4, 4), (2, U, 8, 0)]
    lead = b"\0" * 16
    case = R.pack([lead, s_align, s_len, s_near, b"", s_known, s_last], [[], recs_align, recs_len, recs_near, [], recs_known, recs_last])
    assert int(case[1][1]) % 16 == 0 and int(case[1][-1]) == len(case[0])
    return case, word, big


def test_key_shapes(small_env, small_ctx):
    case, word, big = key_shapes_case()
    per_sentence = E.sentence_words(*case, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(), SMALL_KEYS)
    words = [w for s in per_sentence for w in s]
    assert {word, b"", b"a", b"a\0", b"\0", b"tail", big[:-1] + b"\x01", big[:-1] + b"\x02", big[:-1], b"abcdefgX", b"abcdefgY", b"abcdefg"} <= set(words)
    assert "テスト".encode() in words and b"xyz" not in words and max(len(w) for w in words) == 3072
    listed, absent = half_listed(words)
    for flip in (False, True):   # ... and the other half: every key is looked up listed once and absent once
        vocab = listed if not flip else sorted((set(words) - set(listed)) | absent | {w + b"\1" for w in set(listed) & set(words)})
        want = E.encode_words(per_sentence, vocab, -3)
        hit = int((want[0] != -3).sum())
        assert 0 < hit < len(want[0])
        v = small_env.words().vocabulary(vocab, -3)
        check_ragged(small_ctx, v, case, want)
        v.close()
    # bos and eos around crafted sentences, the empty ones included; an unk_id inside the list's range
    want = E.encode_words(per_sentence, listed, 0, 7, 8)
    v = small_env.words().vocabulary(listed, 0, 7, 8)
    check_ragged(small_ctx, v, case, want)
    v.close()
    # a pool name and a surface with equal bytes are one word: field 0 makes "未知" the word of every unknown record with an id
    name = "未知".encode()
    case2 = R.pack([name + b"--" + name], [[(1, U, 0, 3), (2, U, 2, 1), (0, U, 0, 6), (0, K, 8, 6), (0, U, 6, 2)]])
    want2 = crafted_ids(small_env, case2, {"field": 0}, [b"x", name], 9)
    assert want2[0].tolist() == [1, 1, 1, 1, 9]
    v = small_env.words(field=0).vocabulary([b"x", name], 9)
    check_ragged(small_ctx, v, case2, want2)
    v.close()


# ---- 4. window boundaries / 5. padded ---------------------------------------------------------------------------------------------------------
WINDOW_RECORDS = (0, 1, 63, 64, 65, 127, 128, 129, 1025)
PATTERNS = {"all": lambda k: True, "none": lambda k: False, "alternate": lambda k: k % 2 == 0, "last": lambda k: k % 64 == 63, "first": lambda k: k % 64 == 0}
TEXT = bytes((11 * i + 40) % 200 + 33 for i in range(64))


def window_case(pattern, kept_cls):
    """One sentence per count of WINDOW_RECORDS; record k is kept (class kept_cls, the other class otherwise) by the pattern.  Under KEEP [未知]
    an unknown record is kept and looked up by its bytes; under DROP [未知] a known one is kept and its id comes from the row table."""
    other = K if kept_cls == U else U
    per = []
    for T in WINDOW_RECORDS:
        per.append([(1 + k % 2 if PATTERNS[pattern](k) else 1, kept_cls if PATTERNS[pattern](k) else other, k % 50, 1 + k % 3) for k in range(T)])
    return R.pack([TEXT] * len(WINDOW_RECORDS), per)


def window_vocab(small_env, case, kw):
    words = [w for s in E.sentence_words(*case, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(**kw), SMALL_KEYS) for w in s]
    distinct = sorted(set(words))
    return [b"<pad>", b"<unk>", b"<s>", b"</s>"] + distinct[::2]


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_window_boundaries_ragged_and_padded(small_env, small_ctx, pattern):
    for kw, kept_cls in (({"keep": ("未知",)}, U), ({"drop": ("未知",)}, K)):
        case = window_case(pattern, kept_cls)
        vocab = window_vocab(small_env, case, kw)
        dcase = _Dev(case)
        n = dcase.n
        for bos, eos in ((None, None), (2, 3)):
            want = crafted_ids(small_env, case, kw, vocab, 1, bos, eos)
            L = np.diff(want[1].astype(np.int64))
            extra = (bos is not None) + (eos is not None)
            if pattern == "all":
                assert L.tolist() == [T + extra for T in WINDOW_RECORDS]
                assert 1 in want[0] and (want[0] > 3).any()
            if pattern == "none":
                assert L.tolist() == [extra] * n
            v = small_env.words(**kw).vocabulary(vocab, 1, bos, eos)
            check_ragged(small_ctx, v, dcase, want)
            for width in (1, 2, 63, 64, 65, 200):
                ref = E.padded(want[0], want[1], width, -9, eos)
                if width == 1 and bos is not None and pattern != "none":
                    assert (ref == 3).all(), "bos + eos at width 1: the row is [eos]"
                rc, got, buf, ioff = dev_encode(small_ctx, v, dcase, width=width, pad_id=-9, capacity=n * width, room=n * width + 48)
                assert (rc, got) == (0, len(want[0])), (pattern, width)
                assert np.array_equal(ioff, want[1]), "id_offsets of the padded form are the ragged run's"
                assert np.array_equal(buf[: n * width].reshape(n, width), ref), (pattern, width, bos)
                assert (buf[n * width :] == SENTINEL).all(), "ids behind n x width"
            v.close()


def test_padded_capacity_is_checked_at_enqueue(small_env, small_ctx):
    from kanpyo_amd import _lib

    case = window_case("all", U)
    kw = {"keep": ("未知",)}
    v = small_env.words(**kw).vocabulary(window_vocab(small_env, case, kw), 1)
    n = len(WINDOW_RECORDS)
    with pytest.raises(_lib.KgpuError) as e:
        dev_encode(small_ctx, v, case, width=7, capacity=n * 7 - 1, room=n * 7)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    # a sentence far longer than the row: truncated, never KGPU_ERR_CAPACITY
    long_case = R.pack([TEXT], [[(1, U, k % 50, 1 + k % 3) for k in range(9000)]])
    want = crafted_ids(small_env, long_case, kw, v.words, 1)
    rc, got, buf, ioff = dev_encode(small_ctx, v, long_case, width=64, pad_id=0, capacity=64, room=80)
    assert (rc, got) == (0, 9000) and ioff.tolist() == [0, 9000]
    assert np.array_equal(buf[:64], want[0][:64]) and (buf[64:] == SENTINEL).all()
    v.close()


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------------------------
def test_capacity_device_and_host_forms(env, mixed, small_env, small_ctx):
    from kanpyo_amd import _lib

    case = window_case("alternate", U)
    kw = {"keep": ("未知",)}
    vocab = window_vocab(small_env, case, kw)
    want = crafted_ids(small_env, case, kw, vocab, 1, 2, 3)
    total = len(want[0])
    v = small_env.words(**kw).vocabulary(vocab, 1, 2, 3)
    rc, got, buf, _ = dev_encode(small_ctx, v, case, capacity=total - 1, room=total + 8)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == total and (buf == SENTINEL).all(), "one below the total: the exact count, nothing written"
    rc, got, buf, _ = dev_encode(small_ctx, v, case, capacity=total, room=total + 8)
    assert (rc, got) == (0, total) and np.array_equal(buf[:total], want[0]) and (buf[total:] == SENTINEL).all()
    v.close()
    # the host form: out= one too small (one chunk: nothing written), and without out= the retry
    utf8, offs, tokens = mixed
    offs = offs[:301]
    utf8 = utf8[: int(offs[-1])]
    tokens = (tokens[0], tokens[1][:301])
    vocab, _ = top_half(env, mixed, {})
    want = ref_ids(env, utf8, offs, {}, env.keys, vocab, 1, tokens=tokens)
    total = len(want[0])
    v = env.words().vocabulary(vocab, 1)
    out = (np.full(total - 1, SENTINEL, dtype=np.int32), np.zeros(301, dtype=np.uint64), np.zeros(300, dtype=np.uint8))
    with pytest.raises(_lib.KgpuError) as e:
        v.encode_packed(utf8, offs, out=out)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and str(total) in str(e.value) and (out[0] == SENTINEL).all()
    out = (np.full(total, SENTINEL, dtype=np.int32), np.zeros(301, dtype=np.uint64), np.zeros(300, dtype=np.uint8))
    same(v.encode_packed(utf8, offs, out=out), want)
    # a call of several chunks (2200 sentences: chunks of 1024) with out= one too small: the exact count, and the documented partial delivery --
    # what was written is the ids of whole leading sentences (the chunks that fitted), nothing behind them
    big_utf8, big_offs, big_tokens = mixed
    big_want = ref_ids(env, big_utf8, big_offs, {}, env.keys, vocab, 1, tokens=big_tokens)
    big_total, nb = len(big_want[0]), len(big_offs) - 1
    assert nb > 2 * 1024
    big_out = (np.full(big_total - 1, SENTINEL, dtype=np.int32), np.zeros(nb + 1, dtype=np.uint64), np.zeros(nb, dtype=np.uint8))
    with pytest.raises(_lib.KgpuError) as e:
        v.encode_packed(big_utf8, big_offs, out=big_out)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and f"need {big_total}," in str(e.value)
    written = int(np.flatnonzero(big_out[0] != SENTINEL).max()) + 1 if (big_out[0] != SENTINEL).any() else 0
    assert written < big_total - 1 and written in big_want[1].tolist() and np.array_equal(big_out[0][:written], big_want[0][:written])
    assert (big_out[0][written:] == SENTINEL).all()
    got = C.c_uint64(0)   # a capacity of nothing: the sizing call
    rc = _lib.lib().kgpu_encode_batch(v.handle, utf8.ctypes.data, offs.ctypes.data, 300, None, 0, out[1].ctypes.data, None, C.byref(got))
    assert rc == _lib.KGPU_ERR_CAPACITY and got.value == total
    same(v.encode_packed(utf8, offs), want)
    # without out=: a token per byte is more than the first guess (total // 2 + n + 64 ids) -- the retry takes the count the device reports
    from kanpyo_amd.tokenizer import pack_sentences

    dense = pack_sentences(["a1" * 2000, "a1" * 3])
    want = ref_ids(env, *dense, {}, env.keys, vocab, 1)
    assert len(want[0]) > int(dense[1][-1]) // 2 + 2 + 64
    same(v.encode_packed(*dense), want)
    same(v.encode_text(b"a1" * 2000 + b"\n" + b"a1" * 3 + b"\n"), want)
    v.close()


# ---- 7. one call, chunks and text agree ---------------------------------------------------------------------------------------------------------
def test_one_call_chunks_and_text_agree(env, mixed, monkeypatch):
    from kanpyo_amd.tokenizer import split_lines

    utf8, offs, _ = mixed
    kw = SPECS["drop"]
    vocab, _ = top_half(env, mixed, kw)
    block = b"".join(utf8[int(offs[i]) : int(offs[i + 1])].tobytes() + [b"\r\n", "　\n".encode(), b" \t\n", b"\n"][i % 4] for i in range(len(offs) - 1))
    utf8, offs = split_lines(block)   # (the corpus as read_line + trim_end leave it)
    assert len(offs) - 1 >= 2200
    want = ref_ids(env, utf8, offs, kw, env.keys, vocab, 1, 2, 3)
    v = env.words(**kw).vocabulary(vocab + [b"<s>"], 1, 2, 3)   # (bos_id 2 and eos_id 3 are ordinary entries of the list)
    same(v.encode_packed(utf8, offs), want, "one call")
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "1000")
    same(v.encode_packed(utf8, offs), want, "chunks")
    ids, ioff, st = v.encode_text(block)
    assert len(st) == len(offs) - 1 and not st.any()
    same((ids, ioff), want, "text in chunks")
    monkeypatch.delenv("KGPU_HOST_CHUNK_SENTS")
    same(v.encode_text(block), want, "text")
    v.close()


# ---- 8. forced chains / 9. the chain-rerun recipe ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hooks", [{"KGPU_POOL": "0"}, {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}, {"KGPU_NO_SMALL_CALLS": "1"}])
def test_forced_chains(env, mixed, hooks, monkeypatch):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    for name, val in hooks.items():
        monkeypatch.setenv(name, val)
    e = _Env(env.dict, env.known, env.unk)   # (a fresh handle: the chain is planned per context)
    utf8, offs = pack_sentences(synth.make_corpus(env.sd, 300, 3, "cfg2") + synth.make_corpus(env.sd, 40, 4, "cfg3"))
    for name in ("surface", "field7", "drop"):
        vocab, _ = top_half(env, mixed, SPECS[name])
        v = e.words(**SPECS[name]).vocabulary(vocab, 1, None, 0)
        same(v.encode_packed(utf8, offs), ref_ids(e, utf8, offs, SPECS[name], env.keys, vocab, 1, None, 0), name)
        v.close()


@pytest.mark.parametrize("entry", ["packed", "text"])
def test_chain_rerun_encodes_the_final_records(entry):
    """The recipe of tests/test_gpu_lines.py::test_chain_runs_again_behind_the_render: 14 clean short batches disarm the chain's tail, then a mixed
    block needs it -- the tail runs inside kgpu_ctx_sync, behind the encode queued after the first pass.  The ids are those of the final records."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import split_lines

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    keys = synth.record_surfaces(sd)
    short = [s[:30].replace("\n", "") for s in synth.make_corpus(sd, 600, 9, "cfg2")]
    clean = "".join(s + "\n" for s in short).encode()
    mixed_sents = short[:100] + ["ア" * 900, "漢字かな" * 150] + [s.replace("\n", "") for s in synth.make_corpus(sd, 5, 10, "cfg3")] + short[100:200]
    block = "".join(s + "\n" for s in mixed_sents).encode()
    utf8, offs = split_lines(block)
    exp = e.orc.tokenize_batch(utf8, offs, 8)
    words = E.sentence_words(utf8, offs, exp.tokens, exp.offsets, known, unk, e.nk, e.nu, ref_spec(), keys)
    vocab = [b"<unk>"] + sorted({w for s in words for w in s})[::2]
    v = e.words().vocabulary(vocab, 0)
    enc = (lambda b: v.encode_packed(*split_lines(b))) if entry == "packed" else v.encode_text
    for _ in range(14):
        enc(clean)
    assert e.tok.routing()["tail_reruns"] == 0
    ids, ioff, st = enc(block)
    reruns = e.tok.routing()["tail_reruns"]
    print(f"{entry}: tail_reruns {reruns}")
    assert reruns >= 1, "the mixed batch did not take the tail pass"
    assert not st.any()
    want = E.encode_words(words, vocab, 0)
    assert 0 in want[0] and (want[0] > 0).any()
    same((ids, ioff), want)
    v.close()


# ---- 10. threads and lifetimes -------------------------------------------------------------------------------------------------------------------
def test_eight_threads_on_one_vocab(env, mixed):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    kw = SPECS["field7"]
    vocab, _ = top_half(env, mixed, kw)
    v = env.words(**kw).vocabulary(vocab, 1, 0, None)
    corpora, wants = [], []
    for t in range(8):
        utf8, offs = pack_sentences(synth.make_corpus(env.sd, 300 + 100 * t, 20 + t, "cfg2") + synth.make_corpus(env.sd, 5, 40 + t, "cfg3"))
        corpora.append((utf8, offs))
        wants.append(ref_ids(env, utf8, offs, kw, env.keys, vocab, 1, 0, None))
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


def test_a_vocab_outlives_its_words_handle_and_its_tokenizer():
    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    keys = synth.record_surfaces(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    info = tok.info()
    kw = {"field": 7, "drop": POS_DROP}
    utf8, offs = pack_sentences(synth.make_corpus(sd, 500, 3, "cfg2"))
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 8)
    words = E.sentence_words(utf8, offs, exp.tokens, exp.offsets, known, unk, info["n_morphs"], info["n_unk_morphs"], ref_spec(**kw), keys)
    vocab = [b"<unk>"] + sorted({w for s in words for w in s})[1::2]
    w = tok.words(**kw)
    v = w.vocabulary(vocab, 0, None, 0)
    w.close()
    tok.close()
    want = E.encode_words(words, vocab, 0, None, 0)
    same(v.encode_packed(utf8, offs), want)
    same(v.encode_packed(utf8, offs), want)
    v.close()


# ---- 11. status bytes and empty input -----------------------------------------------------------------------------------------------------------
def test_invalid_utf8_neighbours_and_empty_input(env, mixed):
    from kanpyo_amd.tokenizer import pack_sentences

    word = env.keys[7]
    sents = [b"\xe3\x81", word.encode(), b"\xff", b"", word.encode(), b"\xf8\x88\x80\x80\x80"]
    utf8, offs = pack_sentences(sents)
    for name in ("surface", "field7", "drop"):
        vocab, _ = top_half(env, mixed, SPECS[name])
        for bos, eos in ((None, None), (0, 1)):
            v = env.words(**SPECS[name]).vocabulary(vocab, 1, bos, eos)
            ids, ioff, st = v.encode_packed(utf8, offs)
            assert st.tolist() == [1, 0, 1, 0, 0, 1], name
            one = ref_ids(env, *pack_sentences([word]), SPECS[name], env.keys, vocab, 1)[0].tolist()
            edge = ([] if bos is None else [bos]), ([] if eos is None else [eos])
            rows = [ids[int(ioff[i]) : int(ioff[i + 1])].tolist() for i in range(6)]
            assert rows == [edge[0] + (one if i in (1, 4) else []) + edge[1] for i in range(6)], (name, bos)
            empty = edge[0] + edge[1]
            assert [a.tolist() for a in v.encode([])] == [] and [a.tolist() for a in v.encode([""])] == [empty]
            ids, ioff, st = v.encode_text(b"")
            assert len(ids) == 0 and ioff.tolist() == [0] and len(st) == 0
            ids, ioff, st = v.encode_text(b"\n\n")
            assert ids.tolist() == empty * 2 and ioff.tolist() == [0, len(empty), 2 * len(empty)] and st.tolist() == [0, 0]
            v.close()


# ---- 12. bad records, foreign contexts ---------------------------------------------------------------------------------------------------------
def test_one_bad_record_and_a_foreign_context(small_env, small_ctx):
    from kanpyo_amd import _lib
    from kanpyo_amd.device import DeviceContext

    rng = np.random.default_rng(7)
    case = R.many_case(rng, 1025, small_env.nk, small_env.nu, long_at=(3, 700))
    utf8, offsets, tokens, tok_offsets = case
    per_sentence = E.sentence_words(*case, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(), SMALL_KEYS)
    vocab = [b"<unk>"] + sorted({w for s in per_sentence for w in s})[::2]
    want = E.encode_words(per_sentence, vocab, 0, None, 0)
    total = len(want[0])
    v = small_env.words().vocabulary(vocab, 0, None, 0)
    s, kk = 700, 150
    B = int(offsets[s + 1] - offsets[s])
    r = int(tok_offsets[s]) + kk
    for field, value in (("id", small_env.nk + 1), ("id", -1), ("cls", 3), ("position", B + 1), ("byte_len", B + 1)):
        bad = tokens.copy()
        bad[r] = (1, R.KNOWN, 0, 0, 0, 0)
        bad[r][field] = value
        with pytest.raises(ValueError):
            E.sentence_words(utf8, offsets, bad, tok_offsets, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(), SMALL_KEYS)
        rc, _, _, _ = dev_encode(small_ctx, v, (utf8, offsets, bad, tok_offsets), room=total + 8)
        assert rc == _lib.KGPU_ERR_INVALID_ARG, (field, value)
    back = tok_offsets.copy()
    back[20] = back[19] - 2
    assert dev_encode(small_ctx, v, (utf8, offsets, tokens, back), room=total + 8)[0] == _lib.KGPU_ERR_INVALID_ARG
    check_ragged(small_ctx, v, case, want)   # the handle is still right afterwards
    # a context of another dictionary
    other = _Env(small_env.dict, small_env.known, small_env.unk)
    ctx = DeviceContext(other.tok)
    with pytest.raises(_lib.KgpuError) as e:
        dev_encode(ctx, v, case, room=total + 8)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    ctx.close()
    check_ragged(small_ctx, v, case, want)
    v.close()


# ---- 13. the round trip on the device ----------------------------------------------------------------------------------------------------------
def test_round_trip_count_vocabulary_encode(env, mixed):
    utf8, offs, tokens = mixed
    for name in ("surface", "field7"):
        kw = SPECS[name]
        counts = CR.count(utf8, offs, *tokens, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), env.keys, own_records=True)
        k = env.words(**kw).counter(table_slots=1 << 14, key_bytes=1 << 20)
        k.add_packed(utf8, offs)
        v = k.vocabulary()
        assert v.words == [b"<pad>", b"<unk>"] + [w for w, _ in CR.ordered(counts)] and v.unk_id == 1
        ids, ioff, _ = v.encode_packed(utf8, offs)
        assert np.array_equal(np.bincount(ids, minlength=len(v.words)), [0, 0] + [n for _, n in CR.ordered(counts)]), "the ids' histogram is the counts, in list order"
        same((ids, ioff), ref_ids(env, utf8, offs, kw, env.keys, v.words, 1, tokens=tokens))
        v.close()
        v = k.vocabulary(min_count=2, specials=("<unk>", "<s>", "</s>"), bos="<s>", eos="</s>")
        assert v.words == [b"<unk>", b"<s>", b"</s>"] + [w for w, n in CR.ordered(counts) if n >= 2] and (v.unk_id, v.bos_id, v.eos_id) == (0, 1, 2)
        ids, ioff, _ = v.encode_packed(utf8, offs)
        singles = sum(n for n in counts.values() if n == 1)
        assert singles > 0 and int((ids == 0).sum()) == singles
        same((ids, ioff), ref_ids(env, utf8, offs, kw, env.keys, v.words, 0, 1, 2, tokens=tokens))
        v.close()
        v = k.vocabulary(max_size=100)
        assert v.words == [b"<pad>", b"<unk>"] + [w for w, _ in CR.ordered(counts)][:98]
        v.close()
        k.close()


# ---- 14. encode_tensor -----------------------------------------------------------------------------------------------------------------------------
def test_encode_tensor(env, mixed, tmp_path):
    import torch

    from kanpyo_amd.vocab import Vocab

    utf8, offs, tokens = mixed
    n = 600
    sents = [utf8[int(offs[i]) : int(offs[i + 1])].tobytes() for i in range(n)] + [b"\xff", b""]
    offs2 = np.concatenate([offs[: n + 1], [offs[n], offs[n]]]).astype(np.uint64)   # (the reference skips the invalid line: no tokens)
    toff2 = np.concatenate([tokens[1][: n + 1], [tokens[1][n], tokens[1][n]]]).astype(np.uint64)
    vocab, _ = top_half(env, mixed, {})
    want = ref_ids(env, utf8, offs2, {}, env.keys, vocab, 1, None, 0, tokens=(tokens[0], toff2))
    v = env.words().vocabulary(vocab, 1, None, 0)
    ids, off, st = v.encode_tensor(sents)
    assert ids.is_cuda and off.is_cuda and st.is_cuda and ids.dtype == torch.int32 and off.dtype == torch.int64 and st.dtype == torch.uint8
    assert st.cpu().tolist() == [0] * n + [1, 0]
    same((ids.cpu().numpy(), off.cpu().numpy().astype(np.uint64)), want)
    weight = torch.arange(len(vocab) * 4, dtype=torch.float32, device=ids.device).reshape(len(vocab), 4)
    bag = torch.nn.functional.embedding_bag(ids, weight, off[:-1], mode="sum")
    assert bag.shape == (n + 2, 4)
    row0 = want[0][: int(want[1][1])].astype(np.int64)
    assert np.array_equal(bag[0].cpu().numpy(), weight.cpu().numpy()[row0].sum(axis=0))
    for width in (16, 64):
        pids, lengths, st = v.encode_tensor(sents, width=width, pad_id=-1)
        assert pids.is_cuda and pids.dtype == torch.int32 and tuple(pids.shape) == (n + 2, width) and lengths.dtype == torch.int64
        assert np.array_equal(pids.cpu().numpy(), E.padded(want[0], want[1], width, -1, 0))
        assert np.array_equal(lengths.cpu().numpy(), np.minimum(np.diff(want[1].astype(np.int64)), width))
    # the file form: save, load, the same ids
    path = tmp_path / "vocab.txt"
    v.save(path)
    v2 = Vocab.load(env.words(), path, unk="<unk>", eos="<pad>")
    assert v2.words == v.words and (v2.unk_id, v2.bos_id, v2.eos_id) == (1, None, 0)
    same(v2.encode_packed(utf8, offs2), want)
    with pytest.raises(ValueError):
        Vocab.load(env.words(), path, unk="no such word")
    v.close(); v2.close()


# ---- 15. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_cli(env, mixed, tmp_path):
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
    vocab, _ = top_half(env, mixed, kw)
    vocab = [w for w in vocab if b"\n" not in w] + [b"<s>", b"</s>"]
    vfile = tmp_path / "vocab.txt"
    vfile.write_bytes(b"".join(w + b"\n" for w in vocab))
    bos, eos = len(vocab) - 2, len(vocab) - 1
    text = lambda want: b"".join(" ".join(map(str, want[0][int(want[1][i]) : int(want[1][i + 1])].tolist())).encode() + b"\n" for i in range(len(want[1]) - 1))   # noqa: E731
    plain = ref_ids(env, *split_lines(data), kw, env.keys, vocab, 1)
    edged = ref_ids(env, *split_lines(data), kw, env.keys, vocab, 1, bos, eos)
    assert 1 in plain[0] and (plain[0] > 1).any()
    envv = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "encode", "-c", str(path), "--vocab", str(vfile), "--reading", "--drop", ",".join(POS_DROP)]
    run = lambda extra, inp=data: subprocess.run(cmd + extra, input=inp, capture_output=True, env=envv, cwd=ROOT, timeout=600)   # noqa: E731
    for split in ("host", "device"):   # stdin in small blocks, split on the host and on the device
        r = run(["--block-bytes", "20000", "--split", split])
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == text(plain), split
    r = run(["--bos", "<s>", "--eos", "</s>"])
    assert r.returncode == 0 and r.stdout == text(edged)
    r = run(["--unk", "<no such word>"])
    assert r.returncode == 2 and r.stdout == b"" and "--unk" in r.stderr.decode()
    # an invalid line: status 101, its number on stderr, nothing on stdout; --skip-invalid: the line prints its bos / eos only
    cut = data.index(b"\n", len(data) // 2) + 1
    broken = data[:cut] + b"\xff\xfe\n" + data[cut:]
    bad_line = data[:cut].count(b"\n") + 1
    r = run(["--block-bytes", "20000"], broken)
    assert r.returncode == 101 and r.stdout == b"" and f"line {bad_line}:" in r.stderr.decode()
    r = run(["--block-bytes", "20000", "--skip-invalid", "--split", "device", "--bos", "<s>", "--eos", "</s>"], broken)
    lines = text(edged).split(b"\n")
    lines.insert(bad_line - 1, b"%d %d" % (bos, eos))
    assert r.returncode == 0 and r.stdout == b"\n".join(lines) and f"line {bad_line}:" in r.stderr.decode()
    # INPUT argument: that one string, untrimmed
    one = sents[0] + " "
    want1 = ref_ids(env, *pack_sentences([one]), {}, env.keys, vocab, 1)
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "encode", "-c", str(path), "--vocab", str(vfile), one], capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout == text(want1)
