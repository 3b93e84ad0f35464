"""The host side of the ids with spans (include/kanpyo_gpu.h, "ids with spans") without a device: tests/encode_spans_ref.py against the hand-derived
tests/golden/fixture_encode_spans.json and against the two id references it stands on; the library's host split with piece ends
(kgpu_debug_wordpiece_split_ends, which fills the pool the span kernels read for row-determined words) against the reference's; the tiling property
of a split; the new symbol, the Python names and the argument errors of kgpu_encode_device_spans that are decided before a device is touched."""
import os

import numpy as np

import align_ref as A
import encode_spans_ref as S
import wordpiece_ref as WP
import words_ref as W
from conftest import ROOT, load_golden
from kanpyo_amd import _lib

INC = os.path.join(ROOT, "include")


def lib_split_ends(vocab, words, unk_id, prefix=b"##", max_chars=100):
    from kanpyo_amd.vocab import split_words_ends, wordpiece_opts

    return [(ids.tolist(), [tuple(e) for e in ends.tolist()]) for ids, ends in split_words_ends(vocab, words, unk_id, wordpiece_opts(prefix, max_chars))]


def ref_split_ends(vocab, words, unk_id, prefix=b"##", max_chars=100):
    tabs = WP.tables(vocab, prefix)
    out = []
    for w in words:
        ids, ends = S.piece_ends(tabs, w, max_chars, unk_id)
        assert ids == WP.split_with(tabs, w, max_chars, unk_id), "the span reference's split is not wordpiece_ref's"
        out.append((ids, ends))
    return out


def assert_tiles(word, ids, ends):
    """A word that splits: its pieces' byte ranges are contiguous from 0 to its length, the character ranges from 0 to its character count."""
    starts = WP.char_starts(word)
    assert len(ids) == len(ends) >= 2
    b = c = 0
    for e, ce in ends:
        assert e > b and ce > c and (e == len(word) or e in starts), (word, ends)
        assert ce - c == sum(1 for s in starts if b <= s < e) + (1 if b == 0 and 0 not in starts else 0)
        b, c = e, ce
    assert (b, c) == (len(word), len(starts))


# ---- 1. the host split with ends ------------------------------------------------------------------------------------------------------------------
def test_host_split_ends_on_the_golden_wordpiece_words():
    n_split = 0
    for c in load_golden("fixture_wordpiece.json")["cases"]:
        vocab = [WP.golden_bytes(x) for x in c["list"]]
        unk, prefix = vocab.index(WP.golden_bytes(c["unk"])), WP.golden_bytes(c["prefix"])
        words = [WP.golden_bytes(w["word"]) for w in c["words"]]
        want = ref_split_ends(vocab, words, unk, prefix, c["max_chars"])
        assert [ids for ids, _ in want] == [[vocab.index(p) for p in WP.golden_pieces(w["pieces"])] for w in c["words"]], c["name"]
        assert lib_split_ends(vocab, words, unk, prefix, c["max_chars"]) == want, c["name"]
        for w, (ids, ends) in zip(words, want):
            if len(ids) >= 2:
                assert_tiles(w, ids, ends)
                n_split += 1
    assert n_split >= 10


def test_host_split_ends_on_awkward_words():
    vocab = [b"[UNK]", b"a", "##é".encode(), "##あ".encode(), "##𠮷".encode(), "aé".encode(), "##あ𠮷".encode(), b"##\x81", b"\x81", b"##a"]
    cases = [   # (word, max_word_chars, ids, ends)
        ("aéあ𠮷".encode(), 100, [5, 6], [(3, 2), (10, 4)]),                                  # 1-, 2-, 3- and 4-byte characters in one word
        ("aあé𠮷".encode(), 100, [1, 3, 2, 4], [(1, 1), (4, 2), (6, 3), (10, 4)]),
        ("a𠮷éあ".encode(), 100, [1, 4, 2, 3], [(1, 1), (5, 2), (7, 3), (10, 4)]),
        (b"\x81a", 100, [8, 9], [(1, 1), (2, 2)]),                                            # a stray continuation byte at byte 0 starts a character
        (b"a\x81", 100, [0], [(2, 1)]),                                                       # ... behind a it belongs to a's character: no piece ends before it
        (b"a\x81a", 100, [0], [(3, 2)]),
        (b"", 100, [], []),                                                                   # the empty word
        (b"aaa", 3, [1, 9, 9], [(1, 1), (2, 2), (3, 3)]),                                     # max_word_chars characters ...
        (b"aaaa", 3, [0], [(4, 4)]),                                                          # ... and one more (rule 4b): the one id ends where the word ends
        ("aéx".encode(), 100, [0], [(4, 3)]),                                                 # no split (rule 4d)
        (b"a", 100, [1], [(1, 1)]),
    ]
    for w, max_chars, ids, ends in cases:
        assert ref_split_ends(vocab, [w], 0, max_chars=max_chars) == [(ids, ends)], w
        assert lib_split_ends(vocab, [w], 0, max_chars=max_chars) == [(ids, ends)], w
        if len(ids) >= 2:
            assert_tiles(w, ids, ends)


def test_host_split_ends_on_seeded_random_words():
    rng = np.random.default_rng(19)
    alphabet = ["a", "b", "é", "あ", "ス", "𠮷"]
    word = lambda n: "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))   # noqa: E731
    n_unk = 0
    for prefix, max_chars in ((b"##", 100), (b"##", 5), (b"", 100), (b"@", 100)):
        vocab = [b"[UNK]"]
        for _ in range(120):
            w = word(int(rng.integers(1, 4))).encode()
            w = prefix + w if rng.integers(0, 2) else w
            if w not in vocab:
                vocab.append(w)
        words = [word(int(rng.integers(1, 9))).encode() for _ in range(1200)]
        want = ref_split_ends(vocab, words, 0, prefix, max_chars)
        assert lib_split_ends(vocab, words, 0, prefix, max_chars) == want, (prefix, max_chars)
        split = [(w, r) for w, r in zip(words, want) if len(r[0]) >= 2]
        assert len(split) > 100
        n_unk += sum(r[0] == [0] for r in want)
        for w, (ids, ends) in split:
            assert_tiles(w, ids, ends)
    assert n_unk > 100, "words without a split and words that are too long"


# ---- 2. the golden file pins the reference -----------------------------------------------------------------------------------------------------------
class _Rows:
    """A display table of the golden file: .features(id)."""

    def __init__(self, rows):
        self.rows = rows

    def features(self, tid):
        return self.rows[tid - 1]


def golden_case(c):
    """-> (the arguments of encode_spans_ref.encode for the case, the expected (ids, offsets, spans, index))."""
    text = c["text"].encode()
    tokens = np.zeros(len(c["records"]), dtype=A.TOKEN_DTYPE)
    for i, (tid, cls, pos, blen, start, end) in enumerate(c["records"]):
        tokens[i] = (tid, cls, pos, start, end, blen)
    known = _Rows(c.get("known_features", [["名詞"]] * 3))
    unk = _Rows([["未知"]] * 8)
    spec = W.Spec(W.SURFACE if c["field"] is None else c["field"])
    args = (np.frombuffer(text, dtype=np.uint8), np.array([0, len(text)], dtype=np.uint64), tokens, np.array([0, len(tokens)], dtype=np.uint64), known, unk, 3, 8, spec)
    kw = dict(bos_id=c["bos"], eos_id=c["eos"], wordpiece=c["wordpiece"], edits=None if c["edits"] is None else [[tuple(e) for e in c["edits"]]])
    return args, kw, (c["ids"], [0, len(c["ids"])], c["spans"], c["token_index"])


def test_reference_reproduces_the_golden_file():
    g = load_golden("fixture_encode_spans.json")
    assert g["keys"] == ["テスト", "辞書", "形態素"] and len(g["cases"]) >= 8
    assert sum(c["edits"] is not None for c in g["cases"]) >= 4 and sum(not c["wordpiece"] for c in g["cases"]) >= 2
    for c in g["cases"]:
        args, kw, want = golden_case(c)
        ids, off, spans, index = S.encode(*args, g["keys"], [w.encode() for w in c["list"]], c["unk"], **kw)
        assert (ids.tolist(), off.tolist(), spans.tolist(), index.tolist()) == want, c["name"]
        if c["edits"] is not None:   # the file's edits are what the normaliser gives for its source, and its text is the source's NFKC
            out, status, edits = A.ref_edits(c["source"].encode(), "NFKC")
            assert (out, status, [list(e) for e in edits]) == (c["text"].encode(), 0, c["edits"]), c["name"]
            for (pos, blen, start, end), i in zip(c["spans"], c["token_index"]):   # a span is a slice of the SOURCE at character boundaries
                if i >= 0:
                    assert c["source"].encode()[pos : pos + blen].decode() == c["source"][start:end], c["name"]


def test_reference_padded_form():
    ids, off = np.array([7, 1, 2, 3, 8, 7, 8], dtype=np.int32), np.array([0, 5, 7], dtype=np.uint64)
    spans = np.arange(28, dtype=np.uint32).reshape(7, 4)
    index = np.array([-1, 0, 0, 1, -1, -1, -1], dtype=np.int32)
    pi, ps, px = S.padded(ids, off, spans, index, 3, -9, eos_id=8)
    assert pi.tolist() == [[7, 1, 8], [7, 8, -9]] and px.tolist() == [[-1, 0, -1], [-1, -1, -1]]
    assert ps[0].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [0, 0, 0, 0]] and ps[1].tolist() == [[20, 21, 22, 23], [24, 25, 26, 27], [0, 0, 0, 0]]
    pi, ps, px = S.padded(ids, off, spans, index, 3, -9)   # no eos: the cut row keeps its third element
    assert pi.tolist() == [[7, 1, 2], [7, 8, -9]] and px.tolist() == [[-1, 0, 0], [-1, -1, -1]] and ps[0, 2].tolist() == [8, 9, 10, 11]


# ---- 3. the names and the argument errors that need no device -------------------------------------------------------------------------------------------
def test_new_names_are_there():
    L = _lib.lib()
    assert "kgpu_encode_device_spans" in _lib.SYMBOLS and hasattr(L, "kgpu_encode_device_spans") and L.kgpu_encode_device_spans.argtypes
    with open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8") as f:
        header = f.read()
    assert "kgpu_encode_device_spans(" in header and header.index("ids with spans") > header.index("source alignment")
    assert hasattr(L, "kgpu_debug_wordpiece_split_ends") and "kgpu_debug_wordpiece_split_ends" not in header and "kgpu_debug_wordpiece_split_ends" not in _lib.SYMBOLS
    import inspect

    from kanpyo_amd import cli
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.vocab import Vocab

    assert "return_spans" in inspect.signature(Vocab.encode_tensor).parameters and inspect.signature(Vocab.encode_tensor).parameters["return_spans"].default is False
    assert callable(Vocab.encode_spans) and callable(DeviceContext.encode_spans)
    assert cli.parse_args(["encode", "--vocab", "v"]).offsets is False and cli.parse_args(["encode", "--vocab", "v", "--offsets"]).offsets is True


def test_argument_errors_before_any_device_work():
    """Null pointers, the unpaired edit pointers and the three alignments are refused before the context or the handle is looked at: `c` and `v` below are
    plain zeroed memory."""
    L = _lib.lib()
    bad = _lib.KGPU_ERR_INVALID_ARG
    blob = np.zeros(4096, dtype=np.uint8)
    base = (blob.ctypes.data + 63) & ~63
    c, v, p = base, base + 1024, base + 2048   # p: 64-byte aligned "device" memory that is never touched
    ok = dict(c=c, v=v, utf8=p, off=p, n=1, tok=p, toff=p, edits=None, eoff=None, ids=p, cap=8, width=0, pad=0, ioff=p, spans=p, tix=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.kgpu_encode_device_spans(a["c"], a["v"], a["utf8"], a["off"], a["n"], a["tok"], a["toff"], a["edits"], a["eoff"], a["ids"], a["cap"], a["width"], a["pad"],
                                          a["ioff"], a["spans"], a["tix"])

    for name in ("c", "v", "utf8", "off", "tok", "toff", "ids", "ioff", "spans"):
        assert call(**{name: None}) == bad and b"null argument" in L.kgpu_last_error(), name
    assert call(edits=p) == bad and call(eoff=p) == bad and b"together" in L.kgpu_last_error()
    for shift in (4, 8, 12, 1):
        assert call(spans=p + shift) == bad and b"16-byte" in L.kgpu_last_error(), shift
    for name in ("ids", "tix"):
        for shift in (1, 2, 3):
            assert call(**{name: p + shift}) == bad and b"4-byte" in L.kgpu_last_error(), (name, shift)
