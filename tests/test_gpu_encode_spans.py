"""The ids with spans on the device (include/kanpyo_gpu.h, "ids with spans"; the SPANS instantiations of kgpu_encode.hip and kgpu_wordpiece.hip):
kgpu_encode_device_spans ragged and padded, with and without edit records, Vocab.encode_tensor(return_spans=True), Vocab.encode_spans and
`python -m kanpyo_amd encode --offsets`.  Expected values always come from the oracle's tokens (or crafted records) through tests/encode_spans_ref.py, or
from tests/golden/fixture_encode_spans.json; the edit records of a line come from align_ref.expected_lines (unicodedata over the generator's segments)
-- never from the library.  No tolerance: ids, all n + 1 offsets, every span field and every token index are compared exactly, and on every case the
ids and offsets are also compared with what kgpu_encode_device writes for the same buffers.  The fixtures follow tests/test_gpu_wordpiece.py's pattern."""
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import encode_spans_ref as S
import lines_ref as R
from conftest import ROOT, fixture_dict_parts, load_golden
from record_cases import LIST, SENTINEL, SMALL_KEYS, SPECIALS, _Dev, _Env, bert_like, corpus_of, dev_encode, dev_spans, env, ref_spec, small_ctx  # noqa: F401
from record_cases import check_spans_padded as check_padded
from record_cases import check_spans_ragged as check_ragged
from record_cases import plain_small_env as small_env  # noqa: F401  (env, small_ctx, small_env: the fixtures; this small_env has every EOS reachable)

pytestmark = pytest.mark.gpu

U, K, D = R.UNKNOWN, R.KNOWN, R.DUMMY


def pack6(sent_bytes, per_sentence):
    """lines_ref.pack for records (id, cls, position, byte_len, start, end)."""
    utf8, offsets, tokens, toff = R.pack(sent_bytes, [[r[:4] for r in rs] for rs in per_sentence])
    flat = [r for rs in per_sentence for r in rs]
    if flat:
        tokens["start"], tokens["end"] = [r[4] for r in flat], [r[5] for r in flat]
    return utf8, offsets, tokens, toff


def edit_batch(per_sentence):
    """Per sentence a list of edit 8-tuples -> (edits[EDIT_DTYPE], edit_offsets)."""
    return A.edit_array([e for es in per_sentence for e in es]), np.concatenate([[0], np.cumsum([len(es) for es in per_sentence])]).astype(np.uint64)


def crafted(env, case, vocab, unk, bos=None, eos=None, kw=None, wordpiece=True, edits=None, stats=None, **wp):
    return S.encode(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**(kw or {})), SMALL_KEYS, vocab, unk, bos, eos, wordpiece=wordpiece,
                    edits=edits, stats=stats, **wp)


def _packed(sents):
    from kanpyo_amd.tokenizer import pack_sentences

    return pack_sentences(sents)


# ---- 1. the golden file and the fixture dictionary ---------------------------------------------------------------------------------------------------
def test_golden_file(small_env, small_ctx):
    g = load_golden("fixture_encode_spans.json")
    ran = 0
    for c in g["cases"]:
        if c["field"] is not None:   # (its display table is the file's own: the CPU test covers it)
            continue
        text = c["text"].encode()
        case = pack6([text], [[(tid, cls, pos, blen, start, end) for tid, cls, pos, blen, start, end in c["records"]]])
        vocab = [w.encode() for w in c["list"]]
        want = (np.array(c["ids"], dtype=np.int32), np.array([0, len(c["ids"])], dtype=np.uint64), np.array(c["spans"], dtype=np.uint32).reshape(-1, 4),
                np.array(c["token_index"], dtype=np.int32))
        v = small_env.words().vocabulary(vocab, c["unk"], c["bos"], c["eos"], wordpiece=c["wordpiece"])
        check_ragged(small_ctx, v, case, want, None if c["edits"] is None else edit_batch([[tuple(e) for e in c["edits"]]]), c["name"])
        v.close()
        ran += 1
    assert ran >= 7


def test_fixture_dictionary(small_env, small_ctx):
    sents = ["テストあいうえお辞書形態素", "テスト", "", "あいうえお", "テストテスト"]
    utf8, offs = _packed(sents)
    exp = small_env.orc.tokenize_batch(utf8, offs, 8)
    case = (utf8, offs, exp.tokens, exp.offsets)
    d = _Dev(case)
    for wordpiece, wp in ((True, {}), (True, {"max_chars": 3}), (False, {})):
        for bos, eos in ((None, None), (2, 3)):
            stats = {}
            want = crafted(small_env, case, LIST, 1, bos, eos, wordpiece=wordpiece, stats=stats, **wp)
            if wordpiece and not wp:
                assert (stats["row_split"], stats["text_split"], stats["unk"]) == (4, 2, 1), stats   # テスト x 4 by its row, あいうえお x 2 in the text, 形態素
                first = want[2][int(bos is not None):][:8].tolist()
                assert first == [[0, 3, 0, 1], [3, 3, 1, 2], [6, 3, 2, 3], [9, 3, 3, 4], [12, 3, 4, 5], [15, 3, 5, 6], [18, 6, 6, 8], [24, 6, 8, 10]]
            if wp:
                assert stats["text_split"] == 0 and stats["unk"] == 3, "あいうえお has five characters: rule 4b, one unk_id with the whole span"
            v = small_env.words().vocabulary(LIST, 1, bos, eos, **(dict(wordpiece=True, max_word_chars=wp.get("max_chars", 100)) if wordpiece else {}))
            check_ragged(small_ctx, v, d, want, what=(wordpiece, wp, bos))
            for width in (1, 4, 9, 16):
                check_padded(small_ctx, v, d, want, width, eos)
            v.close()


# ---- 2. crafted records: the slot base carried over a window edge, padded cuts -------------------------------------------------------------------------
TEXT = "テストあいうえお辞書x".encode()   # テスト 0..9 | あいうえお 9..24 | 辞書 24..30 | x 30
KINDS = {   # (id, cls, position, byte_len, start, end)
    "row3": (1, K, 0, 9, 0, 3),        # known id 1, as long as its key: three pieces with their own spans, ends from the pool
    "text4": (0, U, 9, 15, 3, 8),      # the bytes あいうえお without a row: four pieces, ends from the match
    "whole": (2, K, 24, 6, 8, 10),     # 辞書, listed whole
    "unk": (3, K, 30, 1, 10, 11),      # known id 3: 形態素 has no split -> unk_id, the whole span
    "short": (1, K, 3, 6, 1, 3),       # known id 1 with a surface shorter than its key: three pieces, every one the whole span
    "zero": (1, K, 9, 0, 3, 3),        # ... and with byte_len 0
    "empty": (1, U, 30, 0, 10, 10),    # an empty unknown surface: no id
    "eosrec": (0, D, 31, 0, 11, 14),   # the EOS dummy: never an id, but it counts in the token index
}
FILL = ("whole", "row3", "unk", "text4", "empty", "short", "eosrec", "zero")


def window_case(special):
    """Sentences of 63, 64, 65 and 130 records: `special` on lanes 0 and 63 and on the first lane of the next windows, a rotating mix elsewhere."""
    per = [[KINDS[special if k in (0, 63, 64, 128) else FILL[(k + T) % len(FILL)]] for k in range(T)] for T in (63, 64, 65, 130)]
    return pack6([TEXT] * 4, per)


@pytest.mark.parametrize("special", ["row3", "text4"])
def test_window_carry_and_padded_cuts(small_env, small_ctx, special):
    case = window_case(special)
    d = _Dev(case)
    assert case[2][63]["id"] == KINDS[special][0] and int(case[3][2] - case[3][1]) == 64, "a multi-piece token is lane 63 of a full window"
    edits = [[(0, 0, 0, 0, 9, 9, 3, 3)], [], [(9, 9, 3, 3, 3, 5, 1, 2), (24, 26, 8, 9, 6, 6, 2, 2)], [(3, 3, 1, 1, 3, 3, 1, 1)]]
    for bos, eos in ((None, None), (2, 3)):
        for ed in (None, edits):
            stats = {}
            want = crafted(small_env, case, LIST, 1, bos, eos, edits=ed, stats=stats)
            assert stats["row_split"] > 30 and stats["text_split"] > 30 and stats["whole_split"] > 30 and stats["unk"] > 30 and stats["max_records"] == 130
            v = small_env.words().vocabulary(LIST, 1, bos, eos, wordpiece=True)
            check_ragged(small_ctx, v, d, want, None if ed is None else edit_batch(ed), (special, bos))
            if ed is None:
                # widths that cut exactly before a token, inside a row-determined token's pieces and inside a text-keyed token's, by the reference
                L = np.diff(want[1].astype(np.int64))
                kinds = set()
                for width in (1, 2, 3, 5, 6, 7, 64, 65, 131):
                    room = width - (eos is not None)   # the slots bos and the pieces may take in a cut row
                    for s in np.flatnonzero(L > width).tolist():
                        row_i = want[3][int(want[1][s]):][: room + 1]
                        if room >= 1 and len(row_i) > room and row_i[room] == row_i[room - 1] and row_i[room] >= 0:
                            kinds.add("inside " + ("row" if case[2][int(case[3][s]) + int(row_i[room])]["cls"] == K else "text"))
                        else:
                            kinds.add("before")
                    pi, ps, px = check_padded(small_ctx, v, d, want, width, eos)
                    if eos is not None:   # a cut row's last slot is eos with zeros and -1; width 1 holds nothing else
                        cut = L > width
                        assert cut.any() and (pi[cut, -1] == 3).all() and (ps[cut, -1] == 0).all() and (px[cut, -1] == -1).all()
                assert kinds == {"before", "inside row", "inside text"}, kinds
            v.close()


def test_plain_vocabulary_windows(small_env, small_ctx):
    case = window_case("row3")
    d = _Dev(case)
    vocab = SPECIALS + ["テスト".encode(), "辞書".encode()]
    edits = [[(0, 0, 0, 0, 9, 9, 3, 3)], [], [(9, 9, 3, 3, 3, 5, 1, 2), (24, 26, 8, 9, 6, 6, 2, 2)], [(3, 3, 1, 1, 3, 3, 1, 1)]]
    for bos, eos in ((None, None), (2, 3)):
        v = small_env.words().vocabulary(vocab, 1, bos, eos)
        for ed in (None, edits):
            want = crafted(small_env, case, vocab, 1, bos, eos, wordpiece=False, edits=ed)
            check_ragged(small_ctx, v, d, want, None if ed is None else edit_batch(ed))
        want = crafted(small_env, case, vocab, 1, bos, eos, wordpiece=False)
        for width in (1, 2, 63, 64, 65, 200):
            check_padded(small_ctx, v, d, want, width, eos)
        v.close()


# ---- 3. filters, fields, crafted records ------------------------------------------------------------------------------------------------------------------
def test_filters_and_fields(small_env, small_ctx):
    per = [[KINDS[k] for k in ("row3", "text4", "whole", "text4", "row3", "unk", "eosrec")], [KINDS["text4"]], []]
    case = pack6([TEXT] * 3, per)
    # a words handle that drops the unknown tokens' part of speech (feature 0 of every unknown row is 未知): the token indices skip them
    want = crafted(small_env, case, LIST, 1, 2, 3, kw={"drop": ("未知",)})
    assert want[3].tolist() == [-1, 0, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3, 3, 4, 4, 4, 5, -1, -1, 0, 0, 0, 0, -1, -1, -1], "(a record without a row has no feature 0: kept)"
    per2 = [[(1, K, 0, 9, 0, 3), (1, U, 9, 15, 3, 8), (2, K, 24, 6, 8, 10), (2, U, 9, 15, 3, 8), (1, K, 0, 9, 0, 3)]]
    case2 = pack6([TEXT], per2)
    stats = {}
    want2 = crafted(small_env, case2, LIST, 1, 2, 3, kw={"drop": ("未知",)}, stats=stats)
    assert stats["dropped"] == 2 and want2[3].tolist() == [-1, 0, 0, 0, 2, 4, 4, 4, -1]
    v = small_env.words(drop=("未知",)).vocabulary(LIST, 1, 2, 3, wordpiece=True)
    check_ragged(small_ctx, v, case, want)
    check_ragged(small_ctx, v, case2, want2)
    check_padded(small_ctx, v, case2, want2, 5, 3)
    v.close()
    # a feature column (field 0: known id 2 is 名 x 10, the unknown rows 未知; known id 1 has no features and falls back to its key): the ids are pieces, the
    # spans whole tokens -- except the row that falls back to the surface
    vocab = LIST + [w.encode() for w in ("名", "##名", "未", "##知")]
    stats = {}
    want3 = crafted(small_env, case2, vocab, 1, None, 3, kw={"field": 0}, stats=stats)
    assert stats["whole_split"] == 3 and stats["row_split"] == 2 and want3[2][3:13].tolist() == [[9, 15, 3, 8]] * 2 + [[24, 6, 8, 10]] * 8
    v = small_env.words(field=0).vocabulary(vocab, 1, None, 3, wordpiece=True)
    check_ragged(small_ctx, v, case2, want3)
    check_padded(small_ctx, v, case2, want3, 7, 3)
    v.close()


def test_crafted_records(small_env, small_ctx):
    from kanpyo_amd import _lib

    per = [[KINDS["short"], KINDS["zero"], KINDS["row3"], (1, K, 0, 9, 0xFFFFFFFE, 1)], [KINDS["zero"]]]
    case = pack6([TEXT] * 2, per)
    edits = [[(3, 3, 1, 1, 3, 4, 1, 2)], [(9, 9, 3, 3, 3, 3, 1, 1)]]
    v = small_env.words().vocabulary(LIST, 1, None, 3, wordpiece=True)
    for ed in (None, edits):
        want = crafted(small_env, case, LIST, 1, None, 3, edits=ed)
        if ed is None:
            assert want[2][:6].tolist() == [[3, 6, 1, 3]] * 3 + [[9, 0, 3, 3]] * 3, "a record that is not as long as its key: whole spans"
            assert want[2][9:12].tolist() == [[0, 3, 0xFFFFFFFE, 0xFFFFFFFF], [3, 3, 0xFFFFFFFF, 0], [6, 3, 0, 1]], "32-bit, wrapping"
        check_ragged(small_ctx, v, case, want, None if ed is None else edit_batch(ed))
    # token offsets that run backwards: a bad record, the sync says so as kgpu_encode_device's does
    bad = (case[0], case[1], case[2], np.array([0, 4, 3], dtype=np.uint64))
    rc, _, _, _, _, _ = dev_spans(small_ctx, v, bad, room=64)
    assert rc == _lib.KGPU_ERR_INVALID_ARG
    rc, _, _, _ = dev_encode(small_ctx, v, bad, room=64)
    assert rc == _lib.KGPU_ERR_INVALID_ARG
    v.close()


# ---- 4. capacity ---------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_and_no_token_index(small_env, small_ctx):
    from kanpyo_amd import _lib

    case = window_case("text4")
    d = _Dev(case)
    want = crafted(small_env, case, LIST, 1, 2, 3)
    total = len(want[0])
    v = small_env.words().vocabulary(LIST, 1, 2, 3, wordpiece=True)
    rc, got, ids, _, spans, tix = dev_spans(small_ctx, v, d, capacity=total - 1, room=total + 8)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == total, "one below the total: the exact count"
    assert (ids == SENTINEL).all() and (spans == SENTINEL).all() and (tix == SENTINEL).all(), "a call that reports KGPU_ERR_CAPACITY wrote something"
    rc, got, ids, ioff, spans, tix = dev_spans(small_ctx, v, d, capacity=total, room=total + 8, index=False)
    assert (rc, got) == (0, total) and np.array_equal(ids[:total], want[0]) and np.array_equal(spans[:total], want[2]) and np.array_equal(ioff, want[1])
    assert (tix == SENTINEL).all(), "d_token_index == NULL: nothing is written for it"
    v.close()
    plain = SPECIALS + ["テスト".encode()]
    v = small_env.words().vocabulary(plain, 1, 2, 3)
    want = crafted(small_env, case, plain, 1, 2, 3, wordpiece=False)
    rc, got, ids, _, spans, tix = dev_spans(small_ctx, v, d, capacity=len(want[0]) - 1, room=len(want[0]) + 8)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == len(want[0]) and (ids == SENTINEL).all() and (spans == SENTINEL).all() and (tix == SENTINEL).all()
    v.close()


# ---- 5. edits: normalise with edit records, tokenize, encode with spans, all on the device --------------------------------------------------------------------
NORM_KEYS = sorted(["テスト", "辞書", "形態素", "ABC", "(株)", "バス", "ガ", "東京"], key=lambda s: s.encode())
NORM_LIST = SPECIALS + [w.encode() for w in ("テ", "##ス", "##ト", "辞書", "A", "##B", "##C", "(", "##株", "##)", "バ", "ガ", "東", "##京", "ほ", "##か", "##よ", "##り", "##あ")]


@pytest.fixture(scope="module")
def norm_env():
    """The reference's test dictionary with a few more keys: what half-width and full-width text normalises to."""
    from kanpyo_amd import Dict
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = fixture_dict_parts()
    p["sorted_keywords"] = NORM_KEYS
    p["morphs"] = [[i % 3, i % 3, 1000 + 10 * i] for i in range(len(NORM_KEYS))]
    e = _Env(Dict.from_parts(**p), MorphFeatureTable.from_features([["名詞"]] * len(NORM_KEYS)), MorphFeatureTable.from_features([["未知"]] * len(p["unk_morphs"])))
    e.keys = NORM_KEYS
    return e


def ref_pipeline(e, lines, vocab, unk, bos=None, eos=None, kw=None, wordpiece=True, stats=None, form="NFKC"):
    """unicodedata's normalised lines and edit records, the oracle's tokens of those lines, the span reference -> (ids, offsets, spans, index), the status
    bytes, the edits per line.  A line that is not UTF-8 has no records."""
    text, toff, status, edits, eoff = A.expected_lines(lines, form)
    raw, o, eo = text.tobytes(), toff.tolist(), eoff.tolist()
    norm = [b"" if status[i] == 1 else raw[o[i] : o[i + 1]] for i in range(len(lines))]
    utf8, offs = _packed(norm)
    exp = e.orc.tokenize_batch(utf8, offs, 8)
    per_edits = [A.edit_tuples(edits[eo[i] : eo[i + 1]]) for i in range(len(lines))]
    want = S.encode(utf8, offs, exp.tokens, exp.offsets, e.known, e.unk, e.nk, e.nu, ref_spec(**(kw or {})), e.keys, vocab, unk, bos, eos, wordpiece=wordpiece,
                    edits=per_edits, stats=stats)
    return want, status, per_edits


def device_pipeline(ctx, v, lines, width=0, pad_id=0, form="NFKC"):
    """kgpu_normalize_device_aligned, kgpu_tokenize_device, kgpu_encode_device_spans (and kgpu_encode_device on the same buffers) over torch tensors ->
    (ids int32, id_offsets uint64, spans uint32 [.., 4], token_index int32, the plain call's ids and offsets)."""
    import torch

    utf8, offs = _packed(lines)
    n, total = len(lines), int(offs[-1])
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    cap = 11 * total + 16
    d_norm = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_noff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_nst = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_edits = torch.zeros(total * 24 + 24, dtype=torch.uint8, device=dev)
    d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.normalize_aligned(d_utf8.data_ptr(), d_off.data_ptr(), n, d_norm.data_ptr(), cap, d_noff.data_ptr(), d_nst.data_ptr(), d_edits.data_ptr(), total, d_eoff.data_ptr(), form)
    nbytes, _ = ctx.sync_normalize_aligned()
    tcap = nbytes + n + 64
    d_tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.tokenize(d_norm.data_ptr(), d_noff.data_ptr(), n, nbytes, d_tok.data_ptr(), tcap, d_toff.data_ptr(), d_st.data_ptr())
    ctx.sync()
    room = (n * width if width else 4 * nbytes + 2 * n) + 16
    outs = []
    for spans_call in (True, False):
        d_ids = torch.full((room,), SENTINEL, dtype=torch.int32, device=dev)
        d_tix = torch.full((room,), SENTINEL, dtype=torch.int32, device=dev)
        d_spans = torch.full((room, 4), SENTINEL, dtype=torch.int32, device=dev)
        d_ioff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        args = (v, d_norm.data_ptr(), d_noff.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_ids.data_ptr(), room - 16, d_ioff.data_ptr())
        if spans_call:
            ctx.encode_spans(*args, d_spans.data_ptr(), d_tix.data_ptr(), d_edits.data_ptr(), d_eoff.data_ptr(), width=width, pad_id=pad_id)
        else:
            ctx.encode(*args, width=width, pad_id=pad_id)
        count = ctx.sync_lines()
        outs.append((count, d_ids.cpu().numpy(), d_ioff.cpu().numpy().view(np.uint64), d_spans.cpu().numpy().view(np.uint32), d_tix.cpu().numpy()))
    (count, ids, ioff, spans, tix), plain = outs
    assert plain[0] == count and plain[1].tobytes() == ids.tobytes() and plain[2].tobytes() == ioff.tobytes(), "kgpu_encode_device gives other ids for the same buffers"
    used = n * width if width else count
    assert (ids[used:] == SENTINEL).all() and (spans[used:] == SENTINEL).all() and (tix[used:] == SENTINEL).all()
    return count, ids[:used], ioff, spans[:used], tix[:used]


EDIT_LINES = ["ﾃｽﾄ", "ﾊﾞｽ辞書", "㈱", "ＡＢＣ東京", "テスト辞書", b"\xff\xef\xbe\x83", "", "🈀ゟあ", "ｶﾞ㈱ﾃｽﾄ"]


def test_edits_on_the_device(norm_env):
    from kanpyo_amd.device import DeviceContext

    lines = [s if isinstance(s, bytes) else s.encode() for s in EDIT_LINES]
    ctx = DeviceContext(norm_env.tok)
    try:
        for bos, eos in ((None, None), (2, 3)):
            stats = {}
            want, status, per_edits = ref_pipeline(norm_env, lines, NORM_LIST, 1, bos, eos, stats=stats)
            assert status.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] and [len(e) for e in per_edits] == [3, 2, 1, 3, 0, 0, 0, 2, 5]
            assert stats["row_split"] >= 7 and stats["text_split"] >= 1, stats
            o = want[1].tolist()
            body = lambda i: want[2][o[i] + (bos is not None) : o[i + 1] - (eos is not None)].tolist()   # noqa: E731
            assert body(0) == [[0, 3, 0, 1], [3, 3, 1, 2], [6, 3, 2, 3]], "ﾃｽﾄ: every piece one source character"
            assert body(1) == [[0, 6, 0, 2], [6, 3, 2, 3], [9, 6, 3, 5]], "ﾊﾞｽ: バ covers the two-character source segment"
            assert body(2) == [[0, 3, 0, 1]] * 3, "㈱: every piece of (株) covers ㈱"
            assert body(3) == [[0, 3, 0, 1], [3, 3, 1, 2], [6, 3, 2, 3], [9, 3, 3, 4], [12, 3, 4, 5]]
            assert body(4) == [[0, 3, 0, 1], [3, 3, 1, 2], [6, 3, 2, 3], [9, 6, 3, 5]], "a clean line: the spans are the pieces' own"
            assert body(5) == [] and body(6) == [] and o[6] - o[5] == (bos is not None) + (eos is not None), "a line that is not UTF-8, the empty line: specials only"
            assert body(7) == [[0, 4, 0, 1], [0, 4, 0, 1], [4, 3, 1, 2], [4, 3, 1, 2], [7, 3, 2, 3]], "an unknown token through two one-to-two edits"
            v = norm_env.words().vocabulary(NORM_LIST, 1, bos, eos, wordpiece=True)
            count, ids, ioff, spans, tix = device_pipeline(ctx, v, lines)
            assert count == len(want[0]) and np.array_equal(ioff, want[1]) and np.array_equal(ids, want[0])
            assert np.array_equal(spans, want[2]), (spans.tolist(), want[2].tolist())
            assert np.array_equal(tix, want[3])
            for width in (2, 4):
                pi, ps, px = S.padded(*want, width, -7, eos)
                count, ids, ioff, spans, tix = device_pipeline(ctx, v, lines, width=width, pad_id=-7)
                assert count == len(want[0]) and np.array_equal(ioff, want[1])
                assert np.array_equal(ids.reshape(-1, width), pi) and np.array_equal(spans.reshape(-1, width, 4), ps) and np.array_equal(tix.reshape(-1, width), px)
            none = pack6([], [])   # n == 0
            empty = crafted(norm_env, none, NORM_LIST, 1, bos, eos, edits=[])
            assert len(empty[0]) == 0 and empty[1].tolist() == [0]
            check_ragged(ctx, v, none, empty, edit_batch([]))
            check_ragged(ctx, v, none, empty)
            v.close()
            v = norm_env.words().vocabulary(NORM_LIST, 1, bos, eos)   # the plain handle: whole tokens through the edits
            want, _, _ = ref_pipeline(norm_env, lines, NORM_LIST, 1, bos, eos, wordpiece=False)
            count, ids, ioff, spans, tix = device_pipeline(ctx, v, lines)
            assert count == len(want[0]) and np.array_equal(ioff, want[1]) and np.array_equal(ids, want[0]) and np.array_equal(spans, want[2]) and np.array_equal(tix, want[3])
            v.close()
    finally:
        ctx.close()


def test_a_context_of_another_dictionary(small_ctx, norm_env):
    from kanpyo_amd import _lib

    v = norm_env.words().vocabulary(NORM_LIST, 1, wordpiece=True)
    d = _Dev(pack6([TEXT], [[KINDS["row3"]]]))
    with pytest.raises(_lib.KgpuError) as e:
        dev_spans(small_ctx, v, d, room=16)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "dictionary" in str(e.value)
    v.close()


# ---- 6. a mixed corpus on the synthetic dictionary ---------------------------------------------------------------------------------------------------------
DIRT = "ｱｲｳｶｷｸﾞﾟＡＢＣｘｙｚ０１２３"
MIXED_SEED, DROP = 17, ("助詞", "助動詞", "記号")


def dirty(sents, seed):
    """Every tenth character replaced by a half-width kana or mark, or a full-width letter or digit."""
    rng = np.random.default_rng(seed)
    out = []
    for s in sents:
        chars = list(s)
        for i in range(int(rng.integers(0, 10)), len(chars), 10):
            chars[i] = DIRT[int(rng.integers(0, len(DIRT)))]
        out.append("".join(chars).encode())
    return out


@pytest.fixture(scope="module")
def mixed(env):
    """200 keyed, 120 cfg 2 and 30 cfg 3 sentences, every tenth character dirty, with the reference's normalised lines, a BERT-like list of their words and
    the expected output: computed once, never changed."""
    import encode_ref as E

    lines = dirty(corpus_of(env.sd, env.keys, 200, 120, 30, MIXED_SEED), MIXED_SEED)
    text, toff, status, _, _ = A.expected_lines(lines, "NFKC", unchanged_has_none=True)
    assert not status.any()
    exp = env.orc.tokenize_batch(text, toff, 8)
    words = E.sentence_words(text, toff, exp.tokens, exp.offsets, env.known, env.unk, env.nk, env.nu, ref_spec(drop=DROP), env.keys)
    vocab = bert_like(words, 300)
    stats = {}
    want, _, per_edits = ref_pipeline(env, lines, vocab, 1, 2, 3, kw={"drop": DROP}, stats=stats)
    return lines, vocab, want, stats, per_edits


def test_mixed_corpus(env, mixed):
    from kanpyo_amd.device import DeviceContext

    lines, vocab, want, stats, per_edits = mixed
    assert len(lines) == 350
    # not vacuous, by the reference: a row-determined and a text-keyed multi-piece token, an unk_id word, a dropped token, more than 64 records, two edits
    assert stats["row_split"] > 0 and stats["text_split"] > 0 and stats["unk"] > 0 and stats["dropped"] > 0 and stats["max_records"] > 64, stats
    assert max(len(e) for e in per_edits) >= 2 and sum(len(e) for e in per_edits) > 300
    v = env.words(drop=DROP).vocabulary(vocab, 1, 2, 3, wordpiece=True)
    ctx = DeviceContext(env.tok)
    try:
        count, ids, ioff, spans, tix = device_pipeline(ctx, v, lines)
        assert count == len(want[0]) and np.array_equal(ioff, want[1]) and np.array_equal(ids, want[0])
        bad = np.flatnonzero((spans != want[2]).any(axis=1))
        assert bad.size == 0, (bad[:5].tolist(), spans[bad[:5]].tolist(), want[2][bad[:5]].tolist())
        assert np.array_equal(tix, want[3])
        pi, ps, px = S.padded(*want, 24, 0, 3)
        count, ids, ioff, spans, tix = device_pipeline(ctx, v, lines, width=24)
        assert np.array_equal(ids.reshape(-1, 24), pi) and np.array_equal(spans.reshape(-1, 24, 4), ps) and np.array_equal(tix.reshape(-1, 24), px)
    finally:
        ctx.close()
        v.close()


# ---- 7. Python and the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_encode_tensor_and_encode_spans(env, mixed):
    import torch

    lines, vocab, want, _, _ = mixed
    v = env.words(drop=DROP).vocabulary(vocab, 1, 2, 3, wordpiece=True)
    ids, off, st, spans, tix = v.encode_tensor(lines, normalize="NFKC", return_spans=True)
    assert all(t.is_cuda for t in (ids, off, st, spans, tix)) and spans.dtype == torch.int32 and tix.dtype == torch.int32 and tuple(spans.shape) == (len(want[0]), 4)
    assert not st.cpu().numpy().any()
    assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(off.cpu().numpy().astype(np.uint64), want[1])
    assert np.array_equal(spans.cpu().numpy().view(np.uint32), want[2]) and np.array_equal(tix.cpu().numpy(), want[3])
    plain = v.encode_tensor(lines, normalize="NFKC")   # return_spans=False: today's tuple
    assert len(plain) == 3 and np.array_equal(plain[0].cpu().numpy(), want[0])
    pi, ps, px = S.padded(*want, 16, -1, 3)
    ids, lengths, st, spans, tix = v.encode_tensor(lines, width=16, pad_id=-1, normalize="NFKC", return_spans=True)
    assert tuple(spans.shape) == (len(lines), 16, 4) and tuple(tix.shape) == (len(lines), 16)
    assert np.array_equal(ids.cpu().numpy(), pi) and np.array_equal(spans.cpu().numpy().view(np.uint32), ps) and np.array_equal(tix.cpu().numpy(), px)
    assert np.array_equal(lengths.cpu().numpy(), np.minimum(np.diff(want[1].astype(np.int64)), 16))
    rows = v.encode_spans(lines[:40], normalize="NFKC")
    o = want[1].tolist()
    assert len(rows) == 40
    for i, (ri, rs, rx) in enumerate(rows):
        assert rs.dtype == A.SPAN_DTYPE and ri.dtype == np.int32 and rx.dtype == np.int32
        assert np.array_equal(ri, want[0][o[i] : o[i + 1]]) and np.array_equal(rx, want[3][o[i] : o[i + 1]])
        assert np.array_equal(rs.view(np.uint32).reshape(-1, 4), want[2][o[i] : o[i + 1]])
    # an offset_mapping: the characters [start, end) of the source line are its bytes [position, position + byte_len)
    src = lines[3].decode()
    for sp, k in zip(rows[3][1], rows[3][2]):
        if k >= 0:
            assert lines[3][int(sp["position"]) : int(sp["position"]) + int(sp["byte_len"])].decode() == src[int(sp["start"]) : int(sp["end"])]
    v.close()


CLI_INPUT = "ﾃｽﾄ辞書\n㈱バス\n\n"
CLI_WITHOUT_OFFSETS = b"2 4 5 6 7 3\n2 11 12 13 14 5 3\n2 3\n"   # what `encode --wordpiece --normalize nfkc` printed for CLI_INPUT before --offsets existed


def test_cli_offsets(norm_env, tmp_path):
    from kanpyo_amd.dictfile import DictFile, save_dict

    path = tmp_path / "t.dict"
    save_dict(DictFile(norm_env.dict, norm_env.known, norm_env.unk), str(path))
    vfile = tmp_path / "vocab.txt"
    vfile.write_bytes(b"".join(w + b"\n" for w in NORM_LIST))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "encode", "-c", str(path), "--vocab", str(vfile), "--wordpiece", "--unk", "[UNK]", "--bos", "[CLS]", "--eos", "[SEP]",
           "--normalize", "nfkc"]
    lines = [s.encode() for s in CLI_INPUT.split("\n")[:-1]]
    want, _, _ = ref_pipeline(norm_env, lines, NORM_LIST, 1, 2, 3)
    o = want[1].tolist()
    dec = b"".join(" ".join(map(str, want[0][o[i] : o[i + 1]].tolist())).encode() + b"\n" for i in range(len(lines)))
    assert dec == CLI_WITHOUT_OFFSETS, "the recorded output is the reference's"
    r = subprocess.run(cmd, input=CLI_INPUT.encode(), capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == CLI_WITHOUT_OFFSETS, "without --offsets the output is byte for byte what it was"
    r = subprocess.run(cmd + ["--offsets"], input=CLI_INPUT.encode(), capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    expect = []
    for i, ln in enumerate(lines):
        src = ln.decode()
        for e in range(o[i], o[i + 1]):
            sp, k = want[2][e].tolist(), int(want[3][e])
            expect.append("%d\t%d\t%d\t%d\t%s\n" % (want[0][e], sp[2], sp[3], k, src[sp[2] : sp[3]] if k >= 0 else ""))
        expect.append("EOS\n")
    assert r.stdout.decode() == "".join(expect)
    assert r.stdout.decode().startswith("2\t0\t0\t-1\t\n4\t0\t1\t0\tﾃ\n5\t1\t2\t0\tｽ\n6\t2\t3\t0\tﾄ\n7\t3\t5\t1\t辞書\n3\t0\t0\t-1\t\nEOS\n2\t0\t0\t-1\t\n11\t0\t1\t0\t㈱\n")
