"""Tokenizer (reference src/tokenizer.rs:7-45) over the HIP path.

    tokenizer = Tokenizer(dict)          # Tokenizer::new(dict)   src/tokenizer.rs:12-14
    tokens = tokenizer.tokenize("...")   # -> Vec<Token>          src/tokenizer.rs:16-45

plus the batched forms the GPU wants (many sentences per launch).  Everything
computes on the device through include/kanpyo_gpu.h; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from typing import List, Sequence

import numpy as np

from . import _lib
from ._calls import EDIT_DTYPE, SENTENCE_DTYPE, SPAN_DTYPE, TOKEN8_DTYPE, TOKEN_DTYPE, Handle, batch_call, block_bytes, block_call, grown, pack_sentences, packed_input, pinned_empty, ptr, struct_dict  # noqa: F401
from ._probes import concurrent_callers, merge_bench, merge_shards  # noqa: F401  (they lived here once)
from .dict import Dict
from .token import AlignedToken, NBestPath, Token, TokenClass
from .vocab import Vocab

TEXT_UNITS = ("text[uint8]", "text_offsets")   # what the rendering calls name their out= arrays


def merge_status(status: np.ndarray, normalize_status: np.ndarray) -> np.ndarray:
    """The status bytes of a call over normalised text: the tokenizer's, and KGPU_SENT_NOT_NORMALIZED where the normaliser said so and the
    tokenizer said 0 (in place)."""
    status[(status == _lib.KGPU_SENT_OK) & (normalize_status[: status.size] == _lib.KGPU_SENT_NOT_NORMALIZED)] = _lib.KGPU_SENT_NOT_NORMALIZED
    return status


def normalized_call(tokenizer, form, call, utf8=None, offsets=None, block=None, **kw):
    """call(utf8, offsets, **kw) over the input normalised on the device first (Tokenizer.normalize_packed, or normalize_text for a raw block,
    whose lines are then packed): every result's last element is the status array, merged with the normaliser's (merge_status)."""
    text, toff, nstatus = tokenizer.normalize_text(block, form) if block is not None else tokenizer.normalize_packed(utf8, offsets, form)
    result = call(text, toff, **kw)
    merge_status(result[-1] if isinstance(result, tuple) else result, nstatus)
    return result


def normalize_host(data, form="NFKC") -> bytes:
    """kgpu_normalize_host: NFC / NFKC of one string (bytes, or str -> its UTF-8) on the host, by the code and the tables the device runs.
    Needs no device.  Bytes that are not UTF-8, and a line with an oversize segment (include/kanpyo_gpu.h), come back unchanged."""
    raw = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    src = np.frombuffer(raw, dtype=np.uint8)
    out = np.empty(max(src.size * 11, 1), dtype=np.uint8)
    got = C.c_uint64(0)
    _lib.check(_lib.lib().kgpu_normalize_host(_lib.normalize_form(form), ptr(src), src.size, out.ctypes.data, out.size, C.byref(got), None))
    return out[: got.value].tobytes()


def normalize_host_aligned(data, form="NFKC") -> tuple:
    """kgpu_normalize_host_aligned -> (bytes, edits[EDIT_DTYPE]): normalize_host, and one edit record per segment whose bytes changed (include/kanpyo_gpu.h,
    "source alignment").  Needs no device."""
    raw = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    src = np.frombuffer(raw, dtype=np.uint8)
    out = np.empty(max(src.size * 11, 1), dtype=np.uint8)
    edits = np.empty(max(src.size, 1), dtype=EDIT_DTYPE)   # (an edit covers a source byte at least)
    got, ne = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().kgpu_normalize_host_aligned(_lib.normalize_form(form), ptr(src), src.size, out.ctypes.data, out.size, C.byref(got), None,
                                                      edits.ctypes.data, edits.size, C.byref(ne)))
    return out[: got.value].tobytes(), edits[: ne.value]


def _sentence_call(entry, utf8, offsets, terminators, brackets) -> tuple:
    """One sentence split (kgpu_split_sentences_host, or _batch with its handle bound): the first call with room for twice the lines, one more with
    the count the library reports -> (text[uint8], offsets[uint64 S+1], records[SENTENCE_DTYPE S])."""
    utf8, offsets, n, total = packed_input(utf8, offsets)
    opts = _lib.sentence_opts(terminators, brackets)
    out, got = np.empty(max(total, 1), dtype=np.uint8), C.c_uint64(0)
    caps = (2 * n + total // 32 + 64,)
    while caps is not None:
        ooff, recs = np.empty(caps[0] + 1, dtype=np.uint64), np.empty(max(caps[0], 1), dtype=SENTENCE_DTYPE)
        rc = entry(ptr(utf8), offsets.ctypes.data, n, C.byref(opts), out.ctypes.data, ooff.ctypes.data, recs.ctypes.data, caps[0], C.byref(got))
        caps = grown(rc, caps, (got.value,))
    S = got.value
    return out[: int(ooff[S])], ooff[: S + 1], recs[:S]


def split_sentences_host(utf8, offsets, terminators=None, brackets=True) -> tuple:
    """kgpu_split_sentences_host: packed lines cut into sentences (include/kanpyo_gpu.h, "sentences") on the host, by the rule the device runs ->
    (text[uint8], offsets[uint64 S+1], records[SENTENCE_DTYPE S]).  Needs no device; the definition of Tokenizer.split_sentences_packed."""
    return _sentence_call(_lib.lib().kgpu_split_sentences_host, utf8, offsets, terminators, brackets)


def _span_inputs(tokens, tok_offsets, edits, edit_offsets):
    tokens, edits = np.ascontiguousarray(tokens, dtype=TOKEN_DTYPE), np.ascontiguousarray(edits, dtype=EDIT_DTYPE)
    toff, eoff = np.ascontiguousarray(tok_offsets, dtype=np.uint64), np.ascontiguousarray(edit_offsets, dtype=np.uint64)
    if toff.size < 1 or eoff.size != toff.size:
        raise ValueError("tok_offsets and edit_offsets need n+1 entries each")
    if int(toff[-1]) > tokens.size or int(eoff[-1]) > edits.size:
        raise ValueError("the offsets reach past the records")
    return tokens, toff, edits, eoff, np.empty(max(int(toff[-1] - toff[0]), 1), dtype=SPAN_DTYPE)


def source_spans_host(tokens, tok_offsets, edits, edit_offsets) -> np.ndarray:
    """kgpu_source_spans_host -> spans[SPAN_DTYPE], one per record of tokens[tok_offsets[0]:tok_offsets[n]]: the records' position, byte_len, start and
    end in the SOURCE text, through the lines' edits.  Needs no device; the definition of Tokenizer.source_spans."""
    tokens, toff, edits, eoff, spans = _span_inputs(tokens, tok_offsets, edits, edit_offsets)
    _lib.lib().kgpu_source_spans_host(ptr(tokens), toff.ctypes.data, toff.size - 1, ptr(edits), eoff.ctypes.data, spans.ctypes.data)
    return spans[: int(toff[-1] - toff[0])]


def _token_of(raw: bytes, t) -> Token:
    """One 24-byte record of the sentence `raw` as a Token."""
    cls = TokenClass(int(t["cls"]))
    pos, bl = int(t["position"]), int(t["byte_len"])
    return Token(int(t["id"]), cls, pos, int(t["start"]), int(t["end"]), "EOS" if cls == TokenClass.Dummy else raw[pos : pos + bl].decode("utf-8"))


def _sentences(utf8, offs, status, n: int):
    """(i, raw) for each of a packed batch's n sentences, raw being its bytes; UnicodeDecodeError at the first one the device found not to be UTF-8."""
    for i in range(n):
        raw = bytes(utf8[int(offs[i]) : int(offs[i + 1])])
        if status[i] == _lib.KGPU_SENT_INVALID_UTF8:
            raise UnicodeDecodeError("utf-8", raw, 0, 1, "invalid UTF-8 sentence")
        yield i, raw


def _paths_of(utf8, offs, n: int, tokens, poff, toff, costs, status) -> list:
    """Per sentence its NBestPath objects, from the arrays of a paths call (Tokenizer._paths_call)."""
    return [[NBestPath(int(costs[p]), tuple(_token_of(raw, t) for t in tokens[int(toff[p]) : int(toff[p + 1])])) for p in range(int(poff[i]), int(poff[i + 1]))]
            for i, raw in _sentences(utf8, offs, status, n)]


def _token_room(total: int, n: int) -> int:
    """The token records a first call allocates for n sentences of `total` bytes."""
    return total // 2 + n + 64


class Tokenizer(Handle):
    _destroy = "kgpu_dict_destroy"

    def __init__(self, dict: Dict, device: int = 0):
        self.dict = dict  # pub dict: Dict (src/tokenizer.rs:7-9)
        L = _lib.lib()
        b = _lib.DictBlobs()
        self._keep = []
        for name, blob in (
            ("index", dict.index_dict), ("connection", dict.connection_dict), ("morph", dict.morph_dict),
            ("unk", dict.unk_dict), ("char_category", dict.char_category), ("invoke", dict.invoke_list),
            ("group", dict.group_list),
        ):
            a = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
            self._keep.append(a)
            setattr(b, name + "_p", a.ctypes.data if a.size else None)
            setattr(b, name + "_len", a.size)
        h = C.c_void_p()
        _lib.check(L.kgpu_dict_create(C.byref(b), int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def info(self) -> dict:
        i = _lib.DictInfo()
        _lib.check(_lib.lib().kgpu_dict_get_info(self._h, C.byref(i)))
        return struct_dict(i)

    # ---- packed batch: the form the C ABI speaks -------------------------------
    def tokenize_packed(self, utf8: np.ndarray, offsets: np.ndarray, token_capacity: int | None = None, pinned: bool = False,
                        out=None):
        """-> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], status[uint8 n]).
        pinned=True: the output arrays live in pinned host memory (kgpu_host_alloc), so the device-to-host
        copies of a large call run as DMA and overlap its kernels; pass inputs made with `pinned_empty` for
        the same effect on the way in.  out=(tokens, tok_offsets, status): caller-owned result arrays to reuse
        (a fresh 100 MB array costs more in page faults than the tokenization)."""
        return batch_call(partial(_lib.lib().kgpu_tokenize_batch, self._h), utf8, offsets, TOKEN_DTYPE, _token_room, ("tokens[TOKEN_DTYPE]", "tok_offsets"),
                          slack=64, alloc=pinned_empty if pinned else np.empty, out=out, capacity=token_capacity)

    # ---- the CLI's output lines (`kanpyo tokenize`, src/bin/kanpyo.rs:174-197) ------
    def set_features(self, known, unk) -> None:
        """kgpu_dict_set_features: the display tables -- morph_feature.dict's and unk.dict's MorphFeatureTable (or their bincode
        bytes) -- uploaded once per handle.  The lines calls need them."""
        blobs = [np.frombuffer(t if isinstance(t, (bytes, bytearray)) else t.encode(), dtype=np.uint8) for t in (known, unk)]
        _lib.check(_lib.lib().kgpu_dict_set_features(self._h, *[x for b in blobs for x in (b.ctypes.data if b.size else None, b.size)]))

    # ---- text normalisation (include/kanpyo_gpu.h, "text normalisation"; not an output of the reference) ------
    def normalize_packed(self, utf8: np.ndarray, offsets: np.ndarray, form="NFKC", out=None):
        """kgpu_normalize_batch -> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): line i, NFC or NFKC, is
        text[text_offsets[i]:text_offsets[i+1]] -- the (utf8, offsets) pair every packed call takes.  A line that is not UTF-8 (status 1) or
        has an oversize segment (status 4) comes back unchanged.  out=(text, text_offsets, status): caller-owned arrays to reuse."""
        return batch_call(partial(_lib.lib().kgpu_normalize_batch, self._h, _lib.normalize_form(form)), utf8, offsets, np.uint8, lambda total, n: total * 2 + 64,
                          TEXT_UNITS, out=out)

    def normalize_packed_aligned(self, utf8: np.ndarray, offsets: np.ndarray, form="NFKC"):
        """kgpu_normalize_batch_aligned -> (text, text_offsets, status, edits[EDIT_DTYPE], edit_offsets[uint64 n+1]): normalize_packed, and line i's edit
        records edits[edit_offsets[i]:edit_offsets[i+1]] -- one per segment whose bytes changed, positions relative to the line -- which
        source_spans maps token records back through."""
        utf8, offsets, n, total = packed_input(utf8, offsets)
        toff, eoff, status = np.empty(n + 1, dtype=np.uint64), np.empty(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
        got, ne = C.c_uint64(0), C.c_uint64(0)
        caps = (total * 2 + 64, total // 4 + 64)
        while caps is not None:   # (either size may be the one that did not fit: once more with both)
            text, edits = np.empty(max(caps[0], 1), dtype=np.uint8), np.empty(max(caps[1], 1), dtype=EDIT_DTYPE)
            rc = _lib.lib().kgpu_normalize_batch_aligned(self._h, _lib.normalize_form(form), ptr(utf8), offsets.ctypes.data, n, text.ctypes.data, caps[0], toff.ctypes.data,
                                                         status.ctypes.data, C.byref(got), edits.ctypes.data, caps[1], eoff.ctypes.data, C.byref(ne))
            caps = grown(rc, caps, (got.value, ne.value))
        return text[: got.value], toff, status[:n], edits[: ne.value], eoff

    def source_spans(self, tokens, tok_offsets, edits, edit_offsets) -> np.ndarray:
        """kgpu_source_spans_batch -> spans[SPAN_DTYPE], one per record of tokens[tok_offsets[0]:tok_offsets[n]], computed on the device: what
        source_spans_host gives."""
        tokens, toff, edits, eoff, spans = _span_inputs(tokens, tok_offsets, edits, edit_offsets)
        _lib.check(_lib.lib().kgpu_source_spans_batch(self._h, ptr(tokens), toff.ctypes.data, toff.size - 1, ptr(edits), eoff.ctypes.data, spans.ctypes.data))
        return spans[: int(toff[-1] - toff[0])]

    def normalize_text(self, block, form="NFKC"):
        """kgpu_normalize_text: a raw block of input (bytes or uint8 array) -> (text, text_offsets, status) as
        normalize_packed(*split_lines(block)) gives them; the split and the trim run on the device too."""
        return block_call(partial(_lib.lib().kgpu_normalize_text, self._h, _lib.normalize_form(form)), block, np.uint8, lambda size: (size * 2 + 64, size // 16 + 1024))

    def normalize(self, sentences: Sequence, form="NFKC") -> list:
        """The sentences normalised on the device: str in gives str out, bytes in gives bytes out (a line that is not UTF-8 comes back as it is)."""
        text, toff, _ = self.normalize_packed(*pack_sentences(sentences), form)
        raw, o = text.tobytes(), toff.tolist()
        return [raw[o[i] : o[i + 1]].decode("utf-8") if isinstance(s, str) else raw[o[i] : o[i + 1]] for i, s in enumerate(sentences)]

    # ---- sentences (include/kanpyo_gpu.h, "sentences"; not an output of the reference) ------
    def split_sentences_packed(self, utf8: np.ndarray, offsets: np.ndarray, terminators=None, brackets=True):
        """kgpu_split_sentences_batch -> (text[uint8], offsets[uint64 S+1], records[SENTENCE_DTYPE S]): the lines cut into sentences on the device --
        the (utf8, offsets) pair every packed call takes -- and for each sentence its line, byte_start and char_start there.  terminators: a str
        or scalar values replacing the default set (at most 16); brackets=False: a terminator inside brackets is a boundary too."""
        return _sentence_call(partial(_lib.lib().kgpu_split_sentences_batch, self._h), utf8, offsets, terminators, brackets)

    def split_sentences(self, lines: Sequence, terminators=None, brackets=True) -> list:
        """Per line the list of its sentences, cut on the device: str in gives str out, bytes in gives bytes out."""
        text, off, recs = self.split_sentences_packed(*pack_sentences(lines), terminators, brackets)
        raw, o = text.tobytes(), off.tolist()
        out = [[] for _ in lines]
        for k, r in enumerate(recs):
            piece = raw[o[k] : o[k + 1]]
            out[int(r["line"])].append(piece.decode("utf-8", "replace") if isinstance(lines[int(r["line"])], str) else piece)
        return out

    def tokenize_lines_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None, normalize=None):
        """-> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's `surface\\tfeatures\\n` lines are
        text[text_offsets[i]:text_offsets[i+1]].  out=(text, text_offsets, status): caller-owned arrays to reuse.
        normalize="NFC" / "NFKC": the input goes through normalize_packed first; the surfaces are those of the NORMALISED text, and a status
        byte is 4 where the normaliser left a line as it was and the tokenizer said 0."""
        if normalize is not None:
            return normalized_call(self, normalize, self.tokenize_lines_packed, utf8, offsets, out=out)
        return batch_call(partial(_lib.lib().kgpu_tokenize_batch_lines, self._h), utf8, offsets, np.uint8, lambda total, n: total * 16 + 8 * n + 64,
                          TEXT_UNITS, out=out)

    def tokenize_text_lines(self, block, normalize=None):
        """kgpu_tokenize_text_lines: a raw block of input (bytes or uint8 array) -> (text, text_offsets, status) as
        tokenize_lines_packed(*split_lines(block)) gives them; the split and the trim run on the device.
        normalize="NFC" / "NFKC": the block goes through normalize_text first (split, trim and normalisation on the device), its lines then
        through tokenize_lines_packed; surfaces and status as there."""
        if normalize is not None:
            return normalized_call(self, normalize, self.tokenize_lines_packed, block=block)
        return block_call(partial(_lib.lib().kgpu_tokenize_text_lines, self._h), block, np.uint8, lambda size: (size * 16 + 64, size // 16 + 1024))

    def tokenize_lines(self, sentences: Sequence) -> bytes:
        """What `kanpyo tokenize` prints for these sentences (str or bytes), one after the other."""
        utf8, offs = pack_sentences(sentences)
        text, _, _ = self.tokenize_lines_packed(utf8, offs)
        return text.tobytes()

    # ---- wakati-gaki: one line of words per sentence (not an output of the reference) ------
    def words(self, field=None, drop=(), keep=(), separator=" ", normalize=None) -> "Words":
        """kgpu_words_create: a Words handle of this dictionary (set_features first).  field: None = the surface, k >= 0 = feature k of the
        token's row (the surface where the row has no such feature, or it is "" or "*"); drop / keep: part-of-speech names compared with
        feature 0 (at most one of the two); separator: one byte, not a newline.  normalize="NFC" / "NFKC": everything rendered, counted or
        encoded through the handle (Words.render*, WordCounts.add*, Vocab.encode_packed / encode_text / encode / encode_tensor) normalises its
        input on the device first; positions and surfaces then refer to the NORMALISED text."""
        return Words(self, field, drop, keep, separator, normalize)

    # ---- the lattice pictures (`kanpyo graphviz`, src/bin/kanpyo.rs:127-148 over src/graphviz.rs:30-163) ------
    def graphviz_packed(self, utf8: np.ndarray, offsets: np.ndarray, dpi: int = 48, full_state: bool = False):
        """kgpu_graphviz_batch -> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's DOT document is
        text[text_offsets[i]:text_offsets[i+1]], byte for byte what the reference's Graphviz::graphviz(dpi, full_state) prints."""
        L, dpi, full = _lib.lib(), int(dpi), 1 if full_state else 0
        return batch_call(lambda u, o, n, *result: L.kgpu_graphviz_batch(self._h, u, o, n, dpi, full, *result), utf8, offsets, np.uint8,
                          lambda total, n: total * 512 + 1024 * n + 64, TEXT_UNITS)

    def graphviz(self, sentences: Sequence, dpi: int = 48, full_state: bool = False) -> List[str]:
        """What `kanpyo graphviz` prints for each of these sentences (str or bytes): one DOT document per sentence."""
        utf8, offs = pack_sentences(sentences)
        text, toff, _ = self.graphviz_packed(utf8, offs, dpi, full_state)
        raw = text.tobytes()
        return [raw[int(toff[i]) : int(toff[i + 1])].decode("utf-8") for i in range(len(toff) - 1)]

    # ---- N-best paths (include/kanpyo_gpu.h, "N-best paths"; not an output of the reference: `mecab -N k`) ------
    def tokenize_nbest_packed(self, utf8: np.ndarray, offsets: np.ndarray, n_best: int, token_capacity: int | None = None, path_capacity: int | None = None):
        """kgpu_tokenize_batch_nbest -> (tokens[TOKEN_DTYPE], path_offsets[uint64 n+1], tok_offsets[uint64 P+1], costs[int32 P], status[uint8 n]):
        sentence i's paths are path_offsets[i]:path_offsets[i+1], best first; path p costs costs[p] and holds tokens[tok_offsets[p]:tok_offsets[p+1]].
        The capacities, when given, are never grown: KGPU_ERR_CAPACITY surfaces as KgpuError."""
        return self._paths_call(_lib.lib().kgpu_tokenize_batch_nbest, lambda k: (k,), utf8, offsets, n_best, token_capacity, path_capacity)

    def _paths_call(self, fn, lead, utf8, offsets, k, token_capacity, path_capacity):
        """A call that gives up to k paths per sentence in N-best's arrays: fn(handle, utf8, offsets, n, *lead(k), tokens, token_capacity, path_offsets,
        tok_offsets, costs, path_capacity, status, &n_paths, &n_tokens), grown and called again on KGPU_ERR_CAPACITY unless a capacity was given."""
        utf8, offsets, n, total = packed_input(utf8, offsets)
        k = int(k)
        fixed = token_capacity is not None or path_capacity is not None
        caps = (_token_room(total, n) * min(max(k, 1), 4) if token_capacity is None else int(token_capacity), n * max(k, 0) if path_capacity is None else int(path_capacity))
        poff, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
        P, T = C.c_uint64(0), C.c_uint64(0)
        while caps is not None:
            tokens, toff, costs = np.empty(max(caps[0], 1), dtype=TOKEN_DTYPE), np.zeros(caps[1] + 1, dtype=np.uint64), np.empty(max(caps[1], 1), dtype=np.int32)
            status[:] = 0
            rc = fn(self._h, ptr(utf8), offsets.ctypes.data, n, *lead(k), tokens.ctypes.data, caps[0], poff.ctypes.data, toff.ctypes.data, costs.ctypes.data, caps[1],
                    status.ctypes.data, C.byref(P), C.byref(T))
            caps = _lib.check(rc) if fixed else grown(rc, caps, (T.value, P.value))
        return tokens[: T.value], poff, toff[: P.value + 1], costs[: P.value], status[:n]

    def tokenize_nbest(self, sentences: Sequence[str], n_best: int, normalize=None) -> List[List[NBestPath]]:
        """Per sentence its n_best lowest-cost paths, best first (fewer where the lattice has fewer; none where EOS is unreachable): NBestPath.cost and
        NBestPath.tokens, the Token objects tokenize_batch gives.  Path 0 holds tokenize_batch's tokens.  normalize="NFC" / "NFKC": the sentences are
        normalised on the device first and every position refers to the NORMALISED sentence, as in tokenize_batch."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        return _paths_of(utf8, offs, len(sentences), *self.tokenize_nbest_packed(utf8, offs, n_best))

    # ---- search and extended modes (include/kanpyo_gpu.h, "search mode"; not an output of the reference: what Kuromoji and Kagome offer for indexing) ------
    def tokenize_mode_packed(self, utf8: np.ndarray, offsets: np.ndarray, mode="search", penalties=None, token_capacity: int | None = None):
        """kgpu_tokenize_batch_mode -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], costs[int32 n], status[uint8 n]): sentence i's records are
        tokens[tok_offsets[i]:tok_offsets[i+1]], the best path under the mode's penalised costs (mode.mode_opts says what mode and penalties may be);
        costs[i] is dp of EOS, 1 << 30 where nothing was accepted.  A given capacity is never grown: KGPU_ERR_CAPACITY surfaces as KgpuError."""
        from .mode import mode_opts

        utf8, offsets, n, total = packed_input(utf8, offsets)
        opts = mode if isinstance(mode, _lib.ModeOpts) else mode_opts(mode, penalties)
        caps = (_token_room(total, n) if token_capacity is None else int(token_capacity),)
        toff, costs, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8)
        T = C.c_uint64(0)
        while caps is not None:
            tokens = np.empty(max(caps[0], 1), dtype=TOKEN_DTYPE)
            status[:] = 0
            rc = _lib.lib().kgpu_tokenize_batch_mode(self._h, ptr(utf8), offsets.ctypes.data, n, C.byref(opts), tokens.ctypes.data, caps[0], toff.ctypes.data,
                                                     costs.ctypes.data, status.ctypes.data, C.byref(T))
            caps = _lib.check(rc) if token_capacity is not None else grown(rc, caps, (T.value,))
        return tokens[: T.value], toff, costs[:n], status[:n]

    def tokenize_mode(self, sentences: Sequence[str], mode="search", penalties=None, normalize=None) -> List[List[Token]]:
        """Per sentence the Token objects of its best path under the mode's penalised costs, as tokenize_batch gives them: mode="normal" gives
        tokenize_batch's, "search" splits long words where the dictionary has their parts, "extended" also cuts unknown words into characters.
        penalties: (kanji_length, kanji_penalty, other_length, other_penalty), default (2, 3000, 7, 1700).  normalize: as in tokenize_nbest."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        tokens, toff, _, status = self.tokenize_mode_packed(utf8, offs, mode, penalties)
        return [[_token_of(raw, t) for t in tokens[int(toff[i]) : int(toff[i + 1])]] for i, raw in _sentences(utf8, offs, status, len(sentences))]

    # ---- user dictionary (include/kanpyo_gpu.h, "user dictionary"; not an output of the reference: `mecab -u`, what Kuromoji and Kagome take beside the system dictionary) ------
    def tokenize_user_packed(self, utf8: np.ndarray, offsets: np.ndarray, userdict, mode="normal", penalties=None, token_capacity: int | None = None):
        """kgpu_tokenize_batch_user -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], costs[int32 n], status[uint8 n]): tokenize_mode_packed's arrays over
        the lattices widened by the matches of `userdict` (a userdict.UserDict made over this tokenizer).  A record of class 3 (TokenClass.User) has
        id = the entry's index + 1.  A given capacity is never grown: KGPU_ERR_CAPACITY surfaces as KgpuError."""
        from .mode import mode_opts

        utf8, offsets, n, total = packed_input(utf8, offsets)
        opts = mode if isinstance(mode, _lib.ModeOpts) else mode_opts(mode, penalties)
        caps = (_token_room(total, n) if token_capacity is None else int(token_capacity),)
        toff, costs, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8)
        T = C.c_uint64(0)
        while caps is not None:
            tokens = np.empty(max(caps[0], 1), dtype=TOKEN_DTYPE)
            status[:] = 0
            rc = _lib.lib().kgpu_tokenize_batch_user(self._h, userdict.handle, ptr(utf8), offsets.ctypes.data, n, C.byref(opts), tokens.ctypes.data, caps[0],
                                                     toff.ctypes.data, costs.ctypes.data, status.ctypes.data, C.byref(T))
            caps = _lib.check(rc) if token_capacity is not None else grown(rc, caps, (T.value,))
        return tokens[: T.value], toff, costs[:n], status[:n]

    def tokenize_user(self, sentences: Sequence[str], userdict, mode="normal", penalties=None, normalize=None) -> List[List[Token]]:
        """Per sentence the Token objects of its best path over the dictionary's words and the user dictionary's, under the mode's penalised costs.  A
        token of class TokenClass.User is an entry of `userdict`: userdict.features(token.id) are its features.  normalize: as in tokenize_nbest (make the
        user dictionary with the same form: UserDict.from_csv(..., normalize=...))."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        tokens, toff, _, status = self.tokenize_user_packed(utf8, offs, userdict, mode, penalties)
        return [[_token_of(raw, t) for t in tokens[int(toff[i]) : int(toff[i + 1])]] for i, raw in _sentences(utf8, offs, status, len(sentences))]

    # ---- lattice probabilities (include/kanpyo_gpu.h, "lattice probabilities"; not an output of the reference: `mecab -m`, `mecab -l --theta`) ------
    def tokenize_marginals_packed(self, utf8: np.ndarray, offsets: np.ndarray, theta: float = _lib.KGPU_THETA_DEFAULT, all_nodes: bool = False, min_prob: float = 0.0,
                                  token_capacity: int | None = None):
        """kgpu_tokenize_batch_marginals -> (tokens[TOKEN_DTYPE], probs[float64 T], on_best[uint8 T], tok_offsets[uint64 n+1], log_z[float64 n],
        best_logprob[float64 n], status[uint8 n]): sentence i's records are tokens[tok_offsets[i]:tok_offsets[i+1]] -- tokenize's own, each with its
        marginal, or with all_nodes every node whose marginal is at least min_prob, in node order, on_best telling tokenize's.  A given capacity is never
        grown: KGPU_ERR_CAPACITY surfaces as KgpuError."""
        utf8, offsets, n, total = packed_input(utf8, offsets)
        sel = _lib.KGPU_MARGINAL_ALL if all_nodes else _lib.KGPU_MARGINAL_BEST
        caps = (_token_room(total, n) * (8 if all_nodes else 1) if token_capacity is None else int(token_capacity),)
        toff, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
        log_z, best_lp = np.zeros(max(n, 1), dtype=np.float64), np.zeros(max(n, 1), dtype=np.float64)
        T = C.c_uint64(0)
        while caps is not None:
            tokens, probs, on_best = np.empty(max(caps[0], 1), dtype=TOKEN_DTYPE), np.empty(max(caps[0], 1), dtype=np.float64), np.empty(max(caps[0], 1), dtype=np.uint8)
            status[:] = 0
            rc = _lib.lib().kgpu_tokenize_batch_marginals(self._h, ptr(utf8), offsets.ctypes.data, n, float(theta), sel, float(min_prob), tokens.ctypes.data, caps[0],
                                                          probs.ctypes.data, on_best.ctypes.data, toff.ctypes.data, log_z.ctypes.data, best_lp.ctypes.data,
                                                          status.ctypes.data, C.byref(T))
            caps = _lib.check(rc) if token_capacity is not None else grown(rc, caps, (T.value,))
        return tokens[: T.value], probs[: T.value], on_best[: T.value], toff, log_z[:n], best_lp[:n], status[:n]

    def tokenize_marginals(self, sentences: Sequence[str], theta: float = _lib.KGPU_THETA_DEFAULT, all_nodes: bool = False, min_prob: float = 0.0, normalize=None) -> list:
        """Per sentence a list of (Token, marginal probability, on tokenize's path) -- tokenize_batch's tokens, or with all_nodes every node whose
        marginal is at least min_prob, in node order.  P(path) is proportional to exp(-theta cost).  normalize: as in tokenize_nbest."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        tokens, probs, on_best, toff, _, _, status = self.tokenize_marginals_packed(utf8, offs, theta, all_nodes, min_prob)
        return [[(_token_of(raw, tokens[r]), float(probs[r]), bool(on_best[r])) for r in range(int(toff[i]), int(toff[i + 1]))]
                for i, raw in _sentences(utf8, offs, status, len(sentences))]

    def tokenize_samples_packed(self, utf8: np.ndarray, offsets: np.ndarray, n_samples: int, seed: int = 0, theta: float = _lib.KGPU_THETA_DEFAULT,
                                token_capacity: int | None = None, path_capacity: int | None = None):
        """kgpu_tokenize_batch_samples -> N-best's arrays (tokens, path_offsets[n+1], tok_offsets[P+1], costs[P], status[n]): per sentence n_samples
        paths drawn with P(path) proportional to exp(-theta cost) (none where EOS is unreachable); the same (seed, sentence index in the call) draws the
        same paths.  The capacities, when given, are never grown."""
        return self._paths_call(_lib.lib().kgpu_tokenize_batch_samples, lambda k: (float(theta), k, int(seed) & (2**64 - 1)), utf8, offsets, n_samples, token_capacity, path_capacity)

    def tokenize_samples(self, sentences: Sequence[str], n_samples: int, seed: int = 0, theta: float = _lib.KGPU_THETA_DEFAULT, normalize=None) -> List[List[NBestPath]]:
        """Per sentence n_samples sampled tokenizations (NBestPath.cost, NBestPath.tokens; none where EOS is unreachable): segmentations for
        subword-regularisation-style augmentation -- another seed, other paths.  normalize: as in tokenize_nbest."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        return _paths_of(utf8, offs, len(sentences), *self.tokenize_samples_packed(utf8, offs, n_samples, seed, theta))

    def routing(self, reset: bool = False) -> dict:
        """kgpu_dict_get_routing: the routing counters of the handle's pooled contexts (small_calls, combined_calls, ...)."""
        r = _lib.Routing()
        _lib.check(_lib.lib().kgpu_dict_get_routing(self._h, C.byref(r), C.sizeof(r), 1 if reset else 0))
        return {n: (list(getattr(r, n)) if n in ("deferred", "redone", "window_handed") else getattr(r, n)) for n, *_ in r._fields_}

    # ---- reference-shaped API --------------------------------------------------
    def tokenize_batch(self, sentences: Sequence[str], normalize=None) -> List[List[Token]]:
        """normalize="NFC" / "NFKC": the sentences are normalised on the device first; Token.position, start, end and surface then refer to
        the NORMALISED sentence -- tokenize_aligned / kgpu_source_spans_* map them back."""
        utf8, offs = pack_sentences(sentences)
        if normalize is not None:
            utf8, offs, _ = self.normalize_packed(utf8, offs, normalize)
        tokens, toff, status = self.tokenize_packed(utf8, offs)
        return [[_token_of(raw, t) for t in tokens[int(toff[i]) : int(toff[i + 1])]] for i, raw in _sentences(utf8, offs, status, len(sentences))]

    def tokenize_aligned(self, sentences: Sequence[str], normalize="NFKC") -> List[List[AlignedToken]]:
        """tokenize_batch(sentences, normalize=...) with every token's place in the sentence AS IT WAS GIVEN: the sentences are normalised with their
        edit records (normalize_packed_aligned), tokenized, and the records mapped back (source_spans) -- all three on the device.  AlignedToken.token
        is tokenize_batch's Token (normalised coordinates and surface); source_position, source_byte_len, source_start, source_end and source_surface
        refer to the source.  A sentence the normaliser left as it was maps to itself."""
        utf8, offs = pack_sentences(sentences)
        text, toff_text, _, edits, eoff = self.normalize_packed_aligned(utf8, offs, normalize)
        tokens, toff, status = self.tokenize_packed(text, toff_text)
        spans = self.source_spans(tokens, toff, edits, eoff)
        out = []
        for i in range(len(sentences)):
            if status[i] == _lib.KGPU_SENT_INVALID_UTF8:
                raise UnicodeDecodeError("utf-8", bytes(utf8[int(offs[i]) : int(offs[i + 1])]), 0, 1, "invalid UTF-8 sentence")
            raw, src = text[int(toff_text[i]) : int(toff_text[i + 1])].tobytes(), utf8[int(offs[i]) : int(offs[i + 1])].tobytes()
            row = []
            for k in range(int(toff[i]), int(toff[i + 1])):
                t, sp = tokens[k], spans[k]
                cls = TokenClass(int(t["cls"]))
                pos, bl, spos, sbl = int(t["position"]), int(t["byte_len"]), int(sp["position"]), int(sp["byte_len"])
                dummy = cls == TokenClass.Dummy
                token = Token(int(t["id"]), cls, pos, int(t["start"]), int(t["end"]), "EOS" if dummy else raw[pos : pos + bl].decode("utf-8"))
                row.append(AlignedToken(token, spos, sbl, int(sp["start"]), int(sp["end"]), "EOS" if dummy else src[spos : spos + sbl].decode("utf-8")))
            out.append(row)
        return out

    def tokenize(self, input: str) -> List[Token]:
        """Tokenizer::tokenize (src/tokenizer.rs:16-45): one sentence == a batch of one."""
        return self.tokenize_batch([input])[0]


def words_spec(field=None, drop=(), keep=(), separator=" "):
    """-> (_lib.WordsSpec, the arrays it points into) for Tokenizer.words' arguments (kgpu_words_spec, include/kanpyo_gpu.h)."""
    if drop and keep:
        raise ValueError("drop and keep exclude each other")
    sep = separator.encode("utf-8") if isinstance(separator, str) else bytes(separator)
    if len(sep) != 1:
        raise ValueError("the separator is one byte")
    listed = list(keep) if keep else list(drop)
    filt = _lib.KGPU_WORDS_KEEP if keep else _lib.KGPU_WORDS_DROP if drop else _lib.KGPU_WORDS_ALL
    names, offs = pack_sentences(listed)
    names = np.ascontiguousarray(names)
    spec = _lib.WordsSpec(C.sizeof(_lib.WordsSpec), _lib.KGPU_WORDS_SURFACE if field is None else int(field), filt, sep[0],
                          names.ctypes.data if names.size else None, offs.ctypes.data, len(listed))
    return spec, (names, offs)


class Words(Handle):
    """A words handle (kgpu_words): a field, a filter and a separator fixed for one Tokenizer.  Every sentence renders to exactly one line --
    the words of its kept tokens joined by the separator, then a newline -- on the device.  Immutable; usable from many threads at once."""

    _destroy = "kgpu_words_destroy"

    def __init__(self, tokenizer: Tokenizer, field=None, drop=(), keep=(), separator=" ", normalize=None):
        self.normalize = None if normalize is None else _lib.normalize_form(normalize)   # (what the handles made from this one inherit)
        spec, keep_alive = words_spec(field, drop, keep, separator)
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_words_create(tokenizer.handle, C.byref(spec), C.byref(h)))
        del keep_alive
        self._h = h
        self.tokenizer = tokenizer

    def render_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None, normalize=None):
        """kgpu_tokenize_batch_words -> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's line is
        text[text_offsets[i]:text_offsets[i+1]].  out=(text, text_offsets, status): caller-owned arrays to reuse.  normalize: None = the form the
        handle was made with (Tokenizer.words)."""
        form = self.normalize if normalize is None else normalize
        if form is not None:
            return normalized_call(self.tokenizer, form, self._render_packed, utf8, offsets, out=out)
        return self._render_packed(utf8, offsets, out=out)

    def _render_packed(self, utf8, offsets, out=None):
        return batch_call(partial(_lib.lib().kgpu_tokenize_batch_words, self._h), utf8, offsets, np.uint8, lambda total, n: total * 2 + n + 64,
                          TEXT_UNITS, out=out)

    def render_text(self, block):
        """kgpu_tokenize_text_words: a raw block of input (bytes or uint8 array) -> (text, text_offsets, status) as
        render_packed(*split_lines(block)) gives them; the split and the trim run on the device."""
        if self.normalize is not None:
            return normalized_call(self.tokenizer, self.normalize, self._render_packed, block=block)
        return block_call(partial(_lib.lib().kgpu_tokenize_text_words, self._h), block, np.uint8, lambda size: (size * 2 + 64, size // 16 + 1024))

    def render(self, sentences: Sequence) -> List[str]:
        """One string of separated words per sentence (str or bytes), without the newline."""
        utf8, offs = pack_sentences(sentences)
        text, toff, _ = self.render_packed(utf8, offs)
        raw = text.tobytes()
        return [raw[int(toff[i]) : int(toff[i + 1]) - 1].decode("utf-8", "replace") for i in range(len(toff) - 1)]

    def counter(self, table_slots=None, key_bytes=None) -> "WordCounts":
        """A WordCounts handle with this handle's field and filter (kgpu_counts_create); None: the header's defaults."""
        return WordCounts(self, table_slots, key_bytes)

    def vocabulary(self, words, unk_id: int, bos_id=None, eos_id=None, wordpiece=False, prefix="##", max_word_chars=100) -> "Vocab":
        """kgpu_vocab_create: a Vocab with this handle's field and filter.  words: the list (str or bytes), id k is words[k]; a kept token whose
        word is not listed gets unk_id (any int32); bos_id / eos_id: None, or the id put in front of / behind every sentence's ids.
        wordpiece=True (kgpu_vocab_create_wordpiece): a word outside the list is cut into its longest listed pieces, continuation pieces behind `prefix`."""
        return Vocab(self, words, unk_id, bos_id, eos_id, wordpiece, prefix, max_word_chars)


class WordCounts(Handle):
    """A counts handle (kgpu_counts): the word frequencies of everything added to it, accumulated on the device by a Words handle's field and
    filter (include/kanpyo_gpu.h, "word counts").  Any number of threads may add at once; most_common, info and reset take it alone."""

    _destroy = "kgpu_counts_destroy"

    def __init__(self, words: Words, table_slots=None, key_bytes=None):
        opts = _lib.CountsOpts(C.sizeof(_lib.CountsOpts), 0, int(table_slots or 0), int(key_bytes or 0))
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_counts_create(words.handle, C.byref(opts), C.byref(h)))
        self._h = h
        self.words = words

    def add_packed(self, utf8: np.ndarray, offsets: np.ndarray, _normalized: bool = False) -> np.ndarray:
        """kgpu_count_batch -> status[uint8 n].  KgpuError with KGPU_ERR_CAPACITY: some tokens found no room (info()["overflow_tokens"])."""
        if self.words.normalize is not None and not _normalized:
            return normalized_call(self.words.tokenizer, self.words.normalize, self.add_packed, utf8, offsets, _normalized=True)
        utf8, offsets, n, _ = packed_input(utf8, offsets)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(_lib.lib().kgpu_count_batch(self._h, ptr(utf8), offsets.ctypes.data, n, status.ctypes.data))
        return status[:n]

    def add(self, sentences: Sequence) -> np.ndarray:
        """The sentences (str or bytes) tokenized and counted -> their status bytes."""
        return self.add_packed(*pack_sentences(sentences))

    def add_text(self, block) -> np.ndarray:
        """kgpu_count_text: a raw block of input (bytes or uint8 array), split and trimmed on the device -> one status byte per line."""
        if self.words.normalize is not None:
            return normalized_call(self.words.tokenizer, self.words.normalize, self.add_packed, block=block, _normalized=True)
        src = block_bytes(block)
        caps = (src.size // 16 + 1024,)
        n = C.c_uint64(0)
        while caps is not None:   # (a call that was short counted nothing: once more with the exact size)
            status = np.zeros(caps[0], dtype=np.uint8)
            caps = grown(_lib.lib().kgpu_count_text(self._h, ptr(src), src.size, status.ctypes.data, caps[0], C.byref(n)), caps, (n.value,))
        return status[: n.value]

    def most_common(self, n=None) -> List[tuple]:
        """kgpu_counts_read -> [(word bytes, count)], by count descending then bytes ascending; n: the first n of them."""
        top = 0 if n is None else int(n)
        if n is not None and top <= 0:
            return []
        L = _lib.lib()
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        rc = L.kgpu_counts_read(self._h, top, None, 0, None, None, 0, C.byref(ne), C.byref(nb))
        if rc != _lib.KGPU_ERR_CAPACITY:
            _lib.check(rc)
            return []
        words = np.empty(max(int(nb.value), 1), dtype=np.uint8)
        off = np.empty(int(ne.value) + 1, dtype=np.uint64)
        counts = np.empty(max(int(ne.value), 1), dtype=np.uint64)
        _lib.check(L.kgpu_counts_read(self._h, top, words.ctypes.data, words.size, off.ctypes.data, counts.ctypes.data, int(ne.value), C.byref(ne), C.byref(nb)))
        raw, o, c = words.tobytes(), off.tolist(), counts.tolist()
        return [(raw[o[i] : o[i + 1]], c[i]) for i in range(int(ne.value))]

    def info(self) -> dict:
        """kgpu_counts_get_info: tokens_counted, overflow_tokens, sentences, table_slots(_used), key_bytes(_used)."""
        i = _lib.CountsInfo(C.sizeof(_lib.CountsInfo))
        _lib.check(_lib.lib().kgpu_counts_get_info(self._h, C.byref(i)))
        return struct_dict(i)

    def reset(self):
        _lib.check(_lib.lib().kgpu_counts_reset(self._h))

    def vocabulary(self, max_size=None, min_count=1, specials=("<pad>", "<unk>"), unk="<unk>", bos=None, eos=None) -> "Vocab":
        """A Vocab chosen from these counts: specials + [w for w, c in most_common() if c >= min_count][:max_size - len(specials)], words equal
        to a special dropped from the tail.  unk, bos, eos: words of the list (put them among the specials) whose indices become unk_id, bos_id,
        eos_id; bos / eos None: not added.  Vocab.words keeps the list."""
        head = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in specials]
        taken = set(head)
        tail = [w for w, c in self.most_common() if c >= min_count and w not in taken]
        if max_size is not None:
            tail = tail[: max(int(max_size) - len(head), 0)]
        return Vocab.from_words(self.words, head + tail, unk, bos, eos)


def split_lines(block) -> tuple:
    """kgpu_split_lines: the CLI's read_line + trim_end (src/bin/kanpyo.rs:114-122) over a block of input bytes
    -> (uint8 trimmed lines packed, uint64 offsets[n+1]).  Host only: needs no device."""
    src = block_bytes(block)
    n_max = int(np.count_nonzero(src == 10)) + 1
    out = np.empty(max(src.size, 1), dtype=np.uint8)
    offs = np.empty(n_max + 1, dtype=np.uint64)
    n = C.c_uint64(0)
    _lib.check(_lib.lib().kgpu_split_lines(ptr(src), src.size, out.ctypes.data, offs.ctypes.data, offs.size, C.byref(n)))
    k = int(n.value)
    return out[: int(offs[k])], offs[: k + 1]


def tokenize_packed_multi(tokenizers: Sequence[Tokenizer], utf8: np.ndarray, offsets: np.ndarray, token_capacity: int | None = None, out=None, compact: bool = False):
    """kgpu_tokenize_batch_multi: sentence i -> tokenizers[i mod G] (one Tokenizer per device; the same one may appear more than once), results in
    the caller's original order -- byte for byte what Tokenizer.tokenize_packed gives on one device.
    -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], status[uint8 n]).
    compact=True: kgpu_tokenize_batch_multi_compact -> (tokens8[TOKEN8_DTYPE], first[uint32 n x 2], tok_offsets, status); kanpyo_amd.device.expand_tokens
    (kgpu_expand_tokens) restores the 24-byte records where they are consumed."""
    L, G = _lib.lib(), len(tokenizers)
    handles = (C.c_void_p * G)(*[t.handle for t in tokenizers])
    rest = dict(slack=64, out=out, capacity=token_capacity)
    if not compact:
        return batch_call(partial(L.kgpu_tokenize_batch_multi, handles, G), utf8, offsets, TOKEN_DTYPE, _token_room, ("tokens[TOKEN_DTYPE]", "tok_offsets"), **rest)
    utf8, offsets, n, _ = packed_input(utf8, offsets)
    first = np.zeros((max(n, 1), 2), dtype=np.uint32)
    tokens, toff, status = batch_call(lambda u, o, n, t, cap, *more: L.kgpu_tokenize_batch_multi_compact(handles, G, u, o, n, t, cap, first.ctypes.data, *more),
                                      utf8, offsets, TOKEN8_DTYPE, _token_room, ("tokens[TOKEN8_DTYPE]", "tok_offsets"), **rest)
    return tokens, first[:n], toff, status
