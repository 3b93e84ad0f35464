"""What the tests of the record consumers share (the wakati lines, the word counts, the vocabulary and WordPiece ids, the ids with spans): the
environment class, a crafted case in device memory, the device calls on crafted records, the comparisons and the fixtures -- each written once.
A helper module like lines_ref.py: no tests here.  A fixture is imported by the module that requests it and keeps its `module` scope, so every
module has its own instance.  Nothing at import time needs a device."""
import ctypes as C
import random

import numpy as np
import pytest

import count_ref as CR
import encode_ref as E
import encode_spans_ref as S
import wordpiece_ref as WP
import words_ref as W
from conftest import fixture_dict_parts

SENTINEL = 0x5A5A5A5A
SMALL_KEYS = ["テスト", "辞書", "形態素"]               # the keys of the fixture dictionary (small_env's, plain_small_env's, _fixture_env's), by id
SPECIALS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"]   # ids 0..3 of the BERT-like lists
# ids 0..3 are the specials; the pieces of テスト (a known key: from the row), あいうえお (unknown: from the text), 辞書 whole; 形態素 has no split
LIST = SPECIALS + [w.encode() for w in ("テ", "##ス", "##ト", "あ", "##い", "##う", "##えお", "辞書")]
POS_DROP = ("助詞", "助動詞", "記号")
SPECS = {
    "surface": {}, "field0": {"field": 0}, "field7": {"field": 7}, "field8": {"field": 8}, "field40": {"field": 40},
    "drop": {"drop": POS_DROP}, "keep": {"keep": ("感動詞",)},
}
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 3072)   # of the crafted keys of the counts and the ids


def ref_spec(field=None, drop=(), keep=(), separator=" "):
    """Tokenizer.words' arguments as the reference's Spec."""
    return W.Spec(W.SURFACE if field is None else field, W.KEEP if keep else W.DROP if drop else W.ALL, keep or drop, separator)


class _Env:
    """A dictionary with its display tables on the device, its oracle, and Words handles made on demand."""

    def __init__(self, d, known, unk):
        from kanpyo_amd import Tokenizer
        from oracle import oracle

        oracle.build()
        self.dict, self.known, self.unk = d, known, unk
        self.tok = Tokenizer(d)
        self.tok.set_features(known, unk)
        self.orc = oracle.OracleTokenizer.from_dict(d)
        info = self.tok.info()
        self.nk, self.nu = info["n_morphs"], info["n_unk_morphs"]
        self._words = {}

    def words(self, **kw):
        key = repr(sorted(kw.items()))
        if key not in self._words:
            self._words[key] = self.tok.words(**kw)
        return self._words[key]

    def expect(self, utf8, offs, kw, counts=None, tokens=None):
        exp = self.orc.tokenize_batch(utf8, offs, 8) if tokens is None else tokens
        return W.render(utf8, offs, exp.tokens, exp.offsets, self.known, self.unk, self.nk, self.nu, ref_spec(**kw), counts), exp

    def check(self, sents, kw, counts=None, tokens=None):
        from kanpyo_amd.tokenizer import pack_sentences

        utf8, offs = pack_sentences(sents)
        text, toff, status = self.words(**kw).render_packed(utf8, offs)
        (want, want_off), exp = self.expect(utf8, offs, kw, counts, tokens)
        assert np.array_equal(toff, want_off), kw
        assert text.tobytes() == want, kw
        return text, toff, status, exp


def _fixture_env():
    """The fixture dictionary with the display rows of the golden files."""
    from kanpyo_amd import Dict
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = fixture_dict_parts()
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, len(p["unk_morphs"]) + 1)])
    return _Env(Dict.from_parts(**p), known, unk)


def _small_env(**parts):
    """The fixture dictionary, `parts` replaced, with a known row without features, a row with "" and a ten-character name and one
    with a 3400-character (10 200-byte) name."""
    from kanpyo_amd import Dict
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = dict(fixture_dict_parts(), **parts)
    k = MorphFeatureTable([[], [1, 0, 1], [2]], ["", "名" * 10, "長" * 3400])
    u = MorphFeatureTable([[1]] * len(p["unk_morphs"]), ["", "未知"])
    return _Env(Dict.from_parts(**p), k, u)


def synth_env():
    """The 20 000-record dictionary with its display tables, its oracle and its keys by id."""
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    e.sd, e.keys = sd, synth.record_surfaces(sd)
    return e


def _write_dict_dir(d, df, tmp_path):
    """The dictionary's blobs and display tables as the files the C consumers read -> their directory."""
    from kanpyo_amd.dictfile import _unk_prefix_len

    out = tmp_path / "blobs"
    out.mkdir()
    (out / "index.dict").write_bytes(d.index_dict)
    (out / "connection.dict").write_bytes(d.connection_dict)
    (out / "morph.dict").write_bytes(d.morph_dict)
    (out / "unk.dict").write_bytes(d.unk_dict[: _unk_prefix_len(d.unk_dict)] + df.unk_feature_table.encode())
    np.asarray(d.char_category, dtype=np.uint8).tofile(out / "char_category.bin")
    np.asarray(d.invoke_list, dtype=np.uint8).tofile(out / "invoke.bin")
    np.asarray(d.group_list, dtype=np.uint8).tofile(out / "group.bin")
    (out / "morph_feature.dict").write_bytes(df.morph_feature_table.encode())
    (out / "unk_feature.dict").write_bytes(df.unk_feature_table.encode())
    return out


# ---- fixtures (module scope: one instance per importing module) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_env():
    """The small dictionary of test_gpu_lines.py::test_edge_cases: an empty row, a row with "" and a 10 200-byte name, an unreachable EOS."""
    return _small_env(conn_data=[0, 100, 200, 100, -30000, 100, 200, 100, -30000], morphs=[[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]])


@pytest.fixture(scope="module")
def plain_small_env():
    """small_env with the fixture dictionary's own costs: every EOS is reachable.  (A module imports it `as small_env` to request it by that name.)"""
    return _small_env()


@pytest.fixture(scope="module")
def small_ctx(small_env):
    """A context of the importing module's small_env."""
    from kanpyo_amd.device import DeviceContext

    ctx = DeviceContext(small_env.tok)   # never tokenizes
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def env():
    return synth_env()


@pytest.fixture(scope="module")
def mixed(env):
    """2000 cfg 2 sentences and 200 cfg 3 sentences, packed, with the oracle's tokens: computed once, never changed."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(synth.make_corpus(env.sd, 2000, 3, "cfg2") + synth.make_corpus(env.sd, 200, 4, "cfg3"))
    exp = env.orc.tokenize_batch(utf8, offs, 8)
    return utf8, offs, (exp.tokens, exp.offsets)


# ---- corpora and lists with words to split -------------------------------------------------------------------------------------------------------
def corpus_of(sd, keys, n_keyed, n_cfg2, n_cfg3, seed):
    """Sentences strung together from the dictionary's keys of two characters and more (most tokens of the synthetic corpora are one character long:
    nothing to split), then cfg 2 and cfg 3 sentences."""
    from kanpyo_amd import synth

    rng = random.Random(seed)
    longer = [k for k in keys if len(k) >= 2]
    return (["".join(rng.choice(longer) for _ in range(rng.randrange(1, 12))) for _ in range(n_keyed)]
            + synth.make_corpus(sd, n_cfg2, seed, "cfg2") + synth.make_corpus(sd, n_cfg3, seed + 1, "cfg3"))


def characters(words):
    return sorted({w[s:e] for w in words for s, e in zip(WP.char_starts(w), WP.char_starts(w)[1:] + [len(w)])})


def bert_like(per_sentence, top):
    """[PAD] [UNK] [CLS] [SEP], the `top` most frequent words, then every distinct character c of the words and ##c -- except a handful left out."""
    from collections import Counter

    counts = Counter(w for s in per_sentence for w in s)
    order = [w for w, _ in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))]
    chars = characters(order)
    left_out = set(chars[3::25])
    head = [w for w in order[:top] if w not in SPECIALS]
    vocab = SPECIALS + head + [c for c in chars if c not in left_out and c not in set(head)] + [b"##" + c for c in chars if c not in left_out]
    assert len(set(vocab)) == len(vocab) and left_out
    return vocab


# ---- a render's input and destination in device memory ------------------------------------------------------------------------------------------
MARGIN = 64
FILL = 0xAB
CANARY = 0x5A5AC3C35A5AC3C3
OFF_PAD = 8   # canary words on either side of the text offsets


class _Input:
    """A case in device memory.  The byte and record arrays carry a spare element: a batch of empty sentences still needs non-null pointers."""

    def __init__(self, case):
        import torch

        dev = torch.device("cuda", 0)
        utf8, offsets, tokens, tok_offsets = case
        self.n, self.T = len(offsets) - 1, len(tokens)
        u = np.zeros(utf8.size + 16, dtype=np.uint8)
        u[: utf8.size] = utf8
        w = np.zeros((self.T + 1, 6), dtype=np.int32)
        w[: self.T] = np.ascontiguousarray(tokens).view(np.int32).reshape(self.T, 6)
        self.utf8, self.tok = torch.from_numpy(u).to(dev), torch.from_numpy(w).to(dev)
        self.off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev)
        self.toff = torch.from_numpy(np.ascontiguousarray(tok_offsets, dtype=np.uint64).view(np.int64)).to(dev)


class _Dest:
    """capacity bytes `mis` behind a 16-byte boundary, 0xAB all over, margins of MARGIN bytes or more; n + 1 offsets between canary words."""

    def __init__(self, n, capacity, mis):
        import torch

        dev = torch.device("cuda", 0)
        self.n, self.cap, self.lead = n, capacity, MARGIN + mis
        self.buf = torch.full((MARGIN + 16 + capacity + MARGIN,), FILL, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and 0 <= mis < 16
        self.offs = torch.from_numpy(np.full(n + 1 + 2 * OFF_PAD, CANARY, dtype=np.uint64).view(np.int64)).to(dev)
        self.text_ptr, self.offs_ptr = self.buf.data_ptr() + self.lead, self.offs.data_ptr() + 8 * OFF_PAD

    def offsets(self):
        o = self.offs.cpu().numpy().view(np.uint64)
        assert (o[:OFF_PAD] == CANARY).all() and (o[OFF_PAD + self.n + 1 :] == CANARY).all(), "a store outside d_text_offsets[0 .. n]"
        return o[OFF_PAD : OFF_PAD + self.n + 1]

    def margins_intact(self):
        return bool((self.buf[: self.lead] == FILL).all()) and bool((self.buf[self.lead + self.cap :] == FILL).all())

    def holds(self, want: bytes, want_off):
        """d_text[:total] is `want`, every other byte of the allocation is untouched, the offsets are want_off."""
        got = self.buf.cpu().numpy()
        exp = np.full(got.size, FILL, dtype=np.uint8)
        exp[self.lead : self.lead + len(want)] = np.frombuffer(want, dtype=np.uint8)
        if not np.array_equal(got, exp):
            at = int(np.flatnonzero(got != exp)[0]) - self.lead
            raise AssertionError(f"d_text differs first at byte {at} of {len(want)} (negative: the margin in front; beyond: behind the text): "
                                 f"got {got[at + self.lead : at + self.lead + 24].tobytes()!r}, want {exp[at + self.lead : at + self.lead + 24].tobytes()!r}")
        o = self.offsets()
        assert np.array_equal(o, want_off), f"text offsets differ first at {int(np.flatnonzero(o != want_off)[0])}"


def _enqueue(ctx, inp, dest, capacity=None, text_ptr=None):
    import torch

    torch.cuda.synchronize()   # the fills and uploads ran on torch's stream, the render runs on the context's
    ctx.format_lines(inp.utf8.data_ptr(), inp.off.data_ptr(), inp.n, inp.tok.data_ptr(), inp.toff.data_ptr(),
                     dest.text_ptr if text_ptr is None else text_ptr, dest.cap if capacity is None else capacity, dest.offs_ptr)


def _sync(ctx, entry="kgpu_ctx_sync_lines"):
    """The sync entry itself -> (return code, the size it reports): a capacity answer is a result here, not an exception."""
    from kanpyo_amd import _lib

    got = C.c_uint64(0)
    return getattr(_lib.lib(), entry)(ctx._h, C.byref(got)), int(got.value)


# ---- crafted records in device memory -------------------------------------------------------------------------------------------------------------
class _Dev:
    """A crafted case in device memory, byte for byte: NO spare byte behind the text (an empty one gets a dummy allocation)."""

    def __init__(self, case):
        import torch

        dev = torch.device("cuda", 0)
        utf8, offsets, tokens, tok_offsets = case
        self.n = len(offsets) - 1
        self.utf8 = torch.from_numpy(np.ascontiguousarray(utf8).copy() if len(utf8) else np.zeros(1, dtype=np.uint8)).to(dev)
        w = np.zeros((len(tokens) + 1, 6), dtype=np.int32)
        w[: len(tokens)] = np.ascontiguousarray(tokens).view(np.int32).reshape(len(tokens), 6)
        self.tok = torch.from_numpy(w).to(dev)
        self.off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev)
        self.toff = torch.from_numpy(np.ascontiguousarray(tok_offsets, dtype=np.uint64).view(np.int64)).to(dev)
        assert self.utf8.data_ptr() % 16 == 0
        torch.cuda.synchronize()


def dev_count(ctx, counts, case):
    """kgpu_count_words_device + kgpu_ctx_sync_count -> (return code, tokens counted)."""
    d = _Dev(case)
    ctx.count_words(counts, d.utf8.data_ptr(), d.off.data_ptr(), d.n, d.tok.data_ptr(), d.toff.data_ptr())
    return _sync(ctx, "kgpu_ctx_sync_count")


def dev_encode(ctx, v, case, width=0, pad_id=0, capacity=None, room=None):
    """kgpu_encode_device + kgpu_ctx_sync_lines on a crafted case -> (return code, ids reported, the whole destination int32, id_offsets uint64).
    The destination starts ONE int32 behind a 16-byte boundary (d_ids is only 4-byte aligned) and is `room` entries of SENTINEL."""
    import torch

    d = case if isinstance(case, _Dev) else _Dev(case)
    dev = d.utf8.device
    room = (capacity if capacity is not None else 0) + 64 if room is None else room
    buf = torch.full((room + 1,), SENTINEL, dtype=torch.int32, device=dev)
    ioff = torch.full((d.n + 1,), -1, dtype=torch.int64, device=dev)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.encode(v, d.utf8.data_ptr(), d.off.data_ptr(), d.n, d.tok.data_ptr(), d.toff.data_ptr(), buf.data_ptr() + 4, room if capacity is None else capacity,
               ioff.data_ptr(), width=width, pad_id=pad_id)
    rc, got = _sync(ctx)
    return rc, got, buf.cpu().numpy()[1:], ioff.cpu().numpy().view(np.uint64)


def dev_spans(ctx, v, case, edits=None, width=0, pad_id=0, capacity=None, room=None, index=True):
    """kgpu_encode_device_spans + kgpu_ctx_sync_lines on a crafted case -> (return code, ids reported, ids int32 [room], id_offsets uint64, spans uint32
    [room, 4], token_index int32 [room]).  All three destinations are `room` entries of SENTINEL; d_ids and d_token_index start ONE int32 behind a 16-byte
    boundary (they are only 4-byte aligned).  edits: (edits[EDIT_DTYPE], edit_offsets) or None."""
    import torch

    d = case if isinstance(case, _Dev) else _Dev(case)
    dev = d.utf8.device
    room = (capacity if capacity is not None else 0) + 64 if room is None else room
    ids = torch.full((room + 1,), SENTINEL, dtype=torch.int32, device=dev)
    tix = torch.full((room + 1,), SENTINEL, dtype=torch.int32, device=dev)
    spans = torch.full((room + 1, 4), SENTINEL, dtype=torch.int32, device=dev)
    ioff = torch.full((d.n + 1,), -1, dtype=torch.int64, device=dev)
    d_ed = d_eoff = None
    if edits is not None:
        raw = np.frombuffer(edits[0].tobytes() + bytes(24), dtype=np.uint8).copy()
        d_ed = torch.from_numpy(raw).to(dev)
        d_eoff = torch.from_numpy(np.ascontiguousarray(edits[1], dtype=np.uint64).view(np.int64)).to(dev)
    assert ids.data_ptr() % 16 == 0 and tix.data_ptr() % 16 == 0 and spans.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.encode_spans(v, d.utf8.data_ptr(), d.off.data_ptr(), d.n, d.tok.data_ptr(), d.toff.data_ptr(), ids.data_ptr() + 4, room if capacity is None else capacity,
                     ioff.data_ptr(), spans.data_ptr(), tix.data_ptr() + 4 if index else 0, d_ed.data_ptr() if d_ed is not None else 0,
                     d_eoff.data_ptr() if d_eoff is not None else 0, width=width, pad_id=pad_id)
    rc, got = _sync(ctx)
    return rc, got, ids.cpu().numpy()[1:], ioff.cpu().numpy().view(np.uint64), spans.cpu().numpy().view(np.uint32)[:room], tix.cpu().numpy()[1:]


def same(got, want, what=""):
    ids, off = got[0], got[1]
    assert ids.dtype == np.int32
    assert np.array_equal(np.asarray(off, dtype=np.uint64), want[1]), what
    assert np.array_equal(ids, want[0]), what


def holds(counts, want, overflow=0):
    """The WordCounts handle's read-out is the reference's, entry for entry; its info agrees with it."""
    got = counts.most_common()
    ref = CR.ordered(want)
    assert len(got) == len(ref), (len(got), len(ref))
    assert got == ref, next((i, g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r)
    info = counts.info()
    assert info["tokens_counted"] == sum(want.values()) and info["overflow_tokens"] == overflow, info
    for top in (1, 3, len(ref), len(ref) + 5):
        assert counts.most_common(top) == ref[:top]
    return info


def crafted_want(env, case, kw, into=None):
    """The reference's Counter for crafted records over the fixture dictionary."""
    return CR.count(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), SMALL_KEYS, into=into)


def crafted_ids(env, case, kw, vocab, unk, bos=None, eos=None):
    """The reference's (ids, id_offsets) of a plain vocabulary for crafted records over the fixture dictionary."""
    return E.encode(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), SMALL_KEYS, vocab, unk, bos, eos)


def check_ragged(ctx, v, case, want):
    """The ragged kgpu_encode_device call against (ids, offsets), nothing behind the total."""
    total = len(want[0])
    rc, n, buf, ioff = dev_encode(ctx, v, case, room=total + 32)
    assert (rc, n) == (0, total)
    assert np.array_equal(ioff, want[1]) and np.array_equal(buf[:total], want[0])
    assert (buf[total:] == SENTINEL).all(), "ids behind the ragged total"


def check_spans_ragged(ctx, v, case, want, edits=None, what=""):
    """The ragged kgpu_encode_spans_device call against (ids, offsets, spans, index), nothing behind the total, and the same ids and offsets as
    kgpu_encode_device."""
    d = case if isinstance(case, _Dev) else _Dev(case)
    total = len(want[0])
    rc, n, ids, ioff, spans, tix = dev_spans(ctx, v, d, edits, room=total + 32)
    assert (rc, n) == (0, total), (what, rc, n, total)
    assert np.array_equal(ioff, want[1]) and np.array_equal(ids[:total], want[0]), (what, ioff.tolist()[:64], ids[:total].tolist()[:64], want[0].tolist()[:64])
    assert np.array_equal(spans[:total], want[2]), (what, spans[:total].tolist(), want[2].tolist())
    assert np.array_equal(tix[:total], want[3]), (what, tix[:total].tolist()[:64], want[3].tolist()[:64])
    assert (ids[total:] == SENTINEL).all() and (spans[total:] == SENTINEL).all() and (tix[total:] == SENTINEL).all(), f"{what}: something behind the ragged total"
    rc, n, plain, poff = dev_encode(ctx, v, d, room=total + 32)
    assert (rc, n) == (0, total) and plain.tobytes() == ids.tobytes() and poff.tobytes() == ioff.tobytes(), f"{what}: kgpu_encode_device gives other ids for the same buffers ({rc}, {n} of {total})"


def check_spans_padded(ctx, v, case, want, width, eos, edits=None, pad_id=-9):
    """The same for the padded form: n rows of `width`, encode_spans_ref.padded's.  -> its (ids, spans, index)"""
    d = case if isinstance(case, _Dev) else _Dev(case)
    n = d.n
    pi, ps, px = S.padded(*want, width, pad_id, eos)
    rc, got, ids, ioff, spans, tix = dev_spans(ctx, v, d, edits, width=width, pad_id=pad_id, capacity=n * width, room=n * width + 48)
    assert (rc, got) == (0, len(want[0])), (width, rc, got, len(want[0]))
    assert np.array_equal(ioff, want[1]), f"width {width}: id_offsets of the padded form are not the ragged run's: {ioff.tolist()[:64]} {want[1].tolist()[:64]}"
    for name, have, ref in (("ids", ids[: n * width].reshape(n, width), pi), ("spans", spans[: n * width].reshape(n, width, 4), ps), ("token index", tix[: n * width].reshape(n, width), px)):
        if not np.array_equal(have, ref):
            row = int(np.argwhere(have != ref)[0][0])
            raise AssertionError(f"width {width}: {name} differ, first in row {row}: device {have[row].tolist()} reference {ref[row].tolist()}")
    assert (ids[n * width:] == SENTINEL).all() and (spans[n * width:] == SENTINEL).all() and (tix[n * width:] == SENTINEL).all(), f"width {width}: something behind n x width"
    rc, got, plain, poff = dev_encode(ctx, v, d, width=width, pad_id=pad_id, capacity=n * width, room=n * width + 48)
    assert rc == 0 and plain.tobytes() == ids.tobytes() and poff.tobytes() == ioff.tobytes(), f"width {width}: kgpu_encode_device gives other ids for the same buffers (rc {rc})"
    return pi, ps, px
