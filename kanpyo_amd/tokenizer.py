"""Tokenizer (reference src/tokenizer.rs:7-45) over the HIP path.

    tokenizer = Tokenizer(dict)          # Tokenizer::new(dict)   src/tokenizer.rs:12-14
    tokens = tokenizer.tokenize("...")   # -> Vec<Token>          src/tokenizer.rs:16-45

plus the batched forms the GPU wants (many sentences per launch).  Everything
computes on the device through include/kanpyo_gpu.h; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib
from .dict import Dict
from .token import Token, TokenClass

# kgpu_token (include/kanpyo_gpu.h)
TOKEN_DTYPE = np.dtype(
    [("id", "<i4"), ("cls", "<u4"), ("position", "<u4"), ("start", "<u4"), ("end", "<u4"), ("byte_len", "<u4")]
)
TOKEN8_DTYPE = np.dtype([("id", "<i4"), ("packed", "<u4")])  # kgpu_token8: cls | chars << 2 | byte_len << 14


def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """np.empty in pinned host memory (kgpu_host_alloc); freed when the array (and its views) are collected."""
    import weakref

    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if not np.isscalar(shape) else int(shape)
    nbytes = max(count * dt.itemsize, 1)
    L = _lib.lib()
    p = L.kgpu_host_alloc(nbytes)
    if not p:
        raise MemoryError(L.kgpu_last_error().decode("utf-8", "replace"))
    buf = (C.c_uint8 * nbytes).from_address(p)
    weakref.finalize(buf, L.kgpu_host_free, p)
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def pack_sentences(sentences: Sequence) -> tuple:
    """list of str/bytes -> (uint8 concatenation, uint64 offsets[n+1])."""
    enc = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in sentences]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        offs[1:] = np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.uint64, count=len(enc)))
    return np.frombuffer(b"".join(enc), dtype=np.uint8), offs


class Tokenizer:
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

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().kgpu_dict_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        i = _lib.DictInfo()
        _lib.check(_lib.lib().kgpu_dict_get_info(self._h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_ if n != "reserved"}

    # ---- packed batch: the form the C ABI speaks -------------------------------
    def tokenize_packed(self, utf8: np.ndarray, offsets: np.ndarray, token_capacity: int | None = None, pinned: bool = False,
                        out=None):
        """-> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], status[uint8 n]).
        pinned=True: the output arrays live in pinned host memory (kgpu_host_alloc), so the device-to-host
        copies of a large call run as DMA and overlap its kernels; pass inputs made with `pinned_empty` for
        the same effect on the way in.  out=(tokens, tok_offsets, status): caller-owned result arrays to reuse
        (a fresh 100 MB array costs more in page faults than the tokenization)."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        total = int(offsets[-1] - offsets[0]) if n else 0
        cap = int(token_capacity) if token_capacity is not None else total // 2 + n + 64
        L = _lib.lib()
        while True:
            if out is not None:
                tokens, toff, status = out
                if tokens.dtype != TOKEN_DTYPE or toff.dtype != np.uint64 or status.dtype != np.uint8 or toff.size < n + 1 or status.size < n:
                    raise ValueError("out=(tokens[TOKEN_DTYPE], tok_offsets[uint64 >= n+1], status[uint8 >= n])")
                cap = tokens.size
                token_capacity = cap  # no silent reallocation of caller-owned arrays
            else:
                alloc = pinned_empty if pinned else np.empty
                tokens = alloc(cap, dtype=TOKEN_DTYPE)
                toff = alloc(n + 1, dtype=np.uint64)
                status = alloc(max(n, 1), dtype=np.uint8)
            status[: max(n, 1)] = 0
            got = C.c_uint64(0)
            rc = L.kgpu_tokenize_batch(
                self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, tokens.ctypes.data, cap,
                toff.ctypes.data, status.ctypes.data, C.byref(got),
            )
            if rc == _lib.KGPU_ERR_CAPACITY and token_capacity is None:
                cap = int(got.value) + 64  # exact size reported by the device
                continue
            _lib.check(rc)
            return tokens[: int(got.value)], toff[: n + 1], status[:n]

    # ---- the CLI's output lines (`kanpyo tokenize`, src/bin/kanpyo.rs:174-197) ------
    def set_features(self, known, unk) -> None:
        """kgpu_dict_set_features: the display tables -- morph_feature.dict's and unk.dict's MorphFeatureTable (or their bincode
        bytes) -- uploaded once per handle.  The lines calls need them."""
        blobs = [np.frombuffer(t if isinstance(t, (bytes, bytearray)) else t.encode(), dtype=np.uint8) for t in (known, unk)]
        _lib.check(_lib.lib().kgpu_dict_set_features(self._h, *[x for b in blobs for x in (b.ctypes.data if b.size else None, b.size)]))

    def tokenize_lines_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None):
        """-> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's `surface\\tfeatures\\n` lines are
        text[text_offsets[i]:text_offsets[i+1]].  out=(text, text_offsets, status): caller-owned arrays to reuse."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        total = int(offsets[-1] - offsets[0]) if n else 0
        cap = total * 16 + 8 * n + 64
        L = _lib.lib()
        while True:
            if out is not None:
                text, toff, status = out
                if text.dtype != np.uint8 or toff.dtype != np.uint64 or status.dtype != np.uint8 or toff.size < n + 1 or status.size < n:
                    raise ValueError("out=(text[uint8], text_offsets[uint64 >= n+1], status[uint8 >= n])")
                cap = text.size
            else:
                text = np.empty(max(cap, 1), dtype=np.uint8)
                toff = np.empty(n + 1, dtype=np.uint64)
                status = np.empty(max(n, 1), dtype=np.uint8)
            status[: max(n, 1)] = 0
            got = C.c_uint64(0)
            rc = L.kgpu_tokenize_batch_lines(self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, text.ctypes.data, cap,
                                             toff.ctypes.data, status.ctypes.data, C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and out is None:
                cap = int(got.value)  # exact size reported by the device
                continue
            _lib.check(rc)
            return text[: int(got.value)], toff[: n + 1], status[:n]

    def tokenize_text_lines(self, block):
        """kgpu_tokenize_text_lines: a raw block of input (bytes or uint8 array) -> (text, text_offsets, status) as
        tokenize_lines_packed(*split_lines(block)) gives them; the split and the trim run on the device."""
        src = _block_bytes(block)
        cap, ocap = src.size * 16 + 64, src.size // 16 + 1024
        L = _lib.lib()
        while True:
            text = np.empty(max(cap, 1), dtype=np.uint8)
            toff = np.empty(ocap, dtype=np.uint64)
            status = np.zeros(ocap, dtype=np.uint8)
            n, got = C.c_uint64(0), C.c_uint64(0)
            rc = L.kgpu_tokenize_text_lines(self._h, src.ctypes.data if src.size else None, src.size, text.ctypes.data, cap, toff.ctypes.data, ocap,
                                            status.ctypes.data, C.byref(n), C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and (int(got.value) > cap or int(n.value) + 1 > ocap):   # exact sizes reported by the device
                cap, ocap = max(cap, int(got.value)), max(ocap, int(n.value) + 1)
                continue
            _lib.check(rc)
            k = int(n.value)
            return text[: int(got.value)], toff[: k + 1], status[:k]

    def tokenize_lines(self, sentences: Sequence) -> bytes:
        """What `kanpyo tokenize` prints for these sentences (str or bytes), one after the other."""
        utf8, offs = pack_sentences(sentences)
        text, _, _ = self.tokenize_lines_packed(utf8, offs)
        return text.tobytes()

    # ---- wakati-gaki: one line of words per sentence (not an output of the reference) ------
    def words(self, field=None, drop=(), keep=(), separator=" ") -> "Words":
        """kgpu_words_create: a Words handle of this dictionary (set_features first).  field: None = the surface, k >= 0 = feature k of the
        token's row (the surface where the row has no such feature, or it is "" or "*"); drop / keep: part-of-speech names compared with
        feature 0 (at most one of the two); separator: one byte, not a newline."""
        return Words(self, field, drop, keep, separator)

    # ---- the lattice pictures (`kanpyo graphviz`, src/bin/kanpyo.rs:127-148 over src/graphviz.rs:30-163) ------
    def graphviz_packed(self, utf8: np.ndarray, offsets: np.ndarray, dpi: int = 48, full_state: bool = False):
        """kgpu_graphviz_batch -> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's DOT document is
        text[text_offsets[i]:text_offsets[i+1]], byte for byte what the reference's Graphviz::graphviz(dpi, full_state) prints."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        total = int(offsets[-1] - offsets[0]) if n else 0
        cap = total * 512 + 1024 * n + 64
        L = _lib.lib()
        while True:
            text = np.empty(max(cap, 1), dtype=np.uint8)
            toff = np.empty(n + 1, dtype=np.uint64)
            status = np.zeros(max(n, 1), dtype=np.uint8)
            got = C.c_uint64(0)
            rc = L.kgpu_graphviz_batch(self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, int(dpi), 1 if full_state else 0,
                                       text.ctypes.data, cap, toff.ctypes.data, status.ctypes.data, C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and int(got.value) > cap:
                cap = int(got.value)  # exact size reported by the device
                continue
            _lib.check(rc)
            return text[: int(got.value)], toff[: n + 1], status[:n]

    def graphviz(self, sentences: Sequence, dpi: int = 48, full_state: bool = False) -> List[str]:
        """What `kanpyo graphviz` prints for each of these sentences (str or bytes): one DOT document per sentence."""
        utf8, offs = pack_sentences(sentences)
        text, toff, _ = self.graphviz_packed(utf8, offs, dpi, full_state)
        raw = text.tobytes()
        return [raw[int(toff[i]) : int(toff[i + 1])].decode("utf-8") for i in range(len(toff) - 1)]

    def routing(self, reset: bool = False) -> dict:
        """kgpu_dict_get_routing: the routing counters of the handle's pooled contexts (small_calls, combined_calls, ...)."""
        r = _lib.Routing()
        _lib.check(_lib.lib().kgpu_dict_get_routing(self._h, C.byref(r), C.sizeof(r), 1 if reset else 0))
        return {n: (list(getattr(r, n)) if n in ("deferred", "redone") else getattr(r, n)) for n, *_ in r._fields_}

    # ---- reference-shaped API --------------------------------------------------
    def tokenize_batch(self, sentences: Sequence[str]) -> List[List[Token]]:
        utf8, offs = pack_sentences(sentences)
        tokens, toff, status = self.tokenize_packed(utf8, offs)
        out = []
        for i, s in enumerate(sentences):
            if status[i] == _lib.KGPU_SENT_INVALID_UTF8:
                raise UnicodeDecodeError("utf-8", bytes(utf8[int(offs[i]) : int(offs[i + 1])]), 0, 1, "invalid UTF-8 sentence")
            raw = utf8[int(offs[i]) : int(offs[i + 1])].tobytes()
            row = []
            for t in tokens[int(toff[i]) : int(toff[i + 1])]:
                cls = TokenClass(int(t["cls"]))
                pos, bl = int(t["position"]), int(t["byte_len"])
                surface = "EOS" if cls == TokenClass.Dummy else raw[pos : pos + bl].decode("utf-8")
                row.append(Token(int(t["id"]), cls, pos, int(t["start"]), int(t["end"]), surface))
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


class Words:
    """A words handle (kgpu_words): a field, a filter and a separator fixed for one Tokenizer.  Every sentence renders to exactly one line --
    the words of its kept tokens joined by the separator, then a newline -- on the device.  Immutable; usable from many threads at once."""

    def __init__(self, tokenizer: Tokenizer, field=None, drop=(), keep=(), separator=" "):
        spec, keep_alive = words_spec(field, drop, keep, separator)
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_words_create(tokenizer.handle, C.byref(spec), C.byref(h)))
        del keep_alive
        self._h = h
        self.tokenizer = tokenizer

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().kgpu_words_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None):
        """kgpu_tokenize_batch_words -> (text[uint8], text_offsets[uint64 n+1], status[uint8 n]): sentence i's line is
        text[text_offsets[i]:text_offsets[i+1]].  out=(text, text_offsets, status): caller-owned arrays to reuse."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        total = int(offsets[-1] - offsets[0]) if n else 0
        cap = total * 2 + n + 64
        L = _lib.lib()
        while True:
            if out is not None:
                text, toff, status = out
                if text.dtype != np.uint8 or toff.dtype != np.uint64 or status.dtype != np.uint8 or toff.size < n + 1 or status.size < n:
                    raise ValueError("out=(text[uint8], text_offsets[uint64 >= n+1], status[uint8 >= n])")
                cap = text.size
            else:
                text = np.empty(max(cap, 1), dtype=np.uint8)
                toff = np.empty(n + 1, dtype=np.uint64)
                status = np.empty(max(n, 1), dtype=np.uint8)
            status[: max(n, 1)] = 0
            got = C.c_uint64(0)
            rc = L.kgpu_tokenize_batch_words(self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, text.ctypes.data, cap,
                                             toff.ctypes.data, status.ctypes.data, C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and out is None:
                cap = int(got.value)  # exact size reported by the device
                continue
            _lib.check(rc)
            return text[: int(got.value)], toff[: n + 1], status[:n]

    def render_text(self, block):
        """kgpu_tokenize_text_words: a raw block of input (bytes or uint8 array) -> (text, text_offsets, status) as
        render_packed(*split_lines(block)) gives them; the split and the trim run on the device."""
        src = _block_bytes(block)
        cap, ocap = src.size * 2 + 64, src.size // 16 + 1024
        L = _lib.lib()
        while True:
            text = np.empty(max(cap, 1), dtype=np.uint8)
            toff = np.empty(ocap, dtype=np.uint64)
            status = np.zeros(ocap, dtype=np.uint8)
            n, got = C.c_uint64(0), C.c_uint64(0)
            rc = L.kgpu_tokenize_text_words(self._h, src.ctypes.data if src.size else None, src.size, text.ctypes.data, cap, toff.ctypes.data, ocap,
                                            status.ctypes.data, C.byref(n), C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and (int(got.value) > cap or int(n.value) + 1 > ocap):   # exact sizes reported by the device
                cap, ocap = max(cap, int(got.value)), max(ocap, int(n.value) + 1)
                continue
            _lib.check(rc)
            k = int(n.value)
            return text[: int(got.value)], toff[: k + 1], status[:k]

    def render(self, sentences: Sequence) -> List[str]:
        """One string of separated words per sentence (str or bytes), without the newline."""
        utf8, offs = pack_sentences(sentences)
        text, toff, _ = self.render_packed(utf8, offs)
        raw = text.tobytes()
        return [raw[int(toff[i]) : int(toff[i + 1]) - 1].decode("utf-8", "replace") for i in range(len(toff) - 1)]


    def counter(self, table_slots=None, key_bytes=None) -> "WordCounts":
        """A WordCounts handle with this handle's field and filter (kgpu_counts_create); None: the header's defaults."""
        return WordCounts(self, table_slots, key_bytes)

    def vocabulary(self, words, unk_id: int, bos_id=None, eos_id=None) -> "Vocab":
        """kgpu_vocab_create: a Vocab with this handle's field and filter.  words: the list (str or bytes), id k is words[k]; a kept token whose
        word is not listed gets unk_id (any int32); bos_id / eos_id: None, or the id put in front of / behind every sentence's ids."""
        from .vocab import Vocab

        return Vocab(self, words, unk_id, bos_id, eos_id)


class WordCounts:
    """A counts handle (kgpu_counts): the word frequencies of everything added to it, accumulated on the device by a Words handle's field and
    filter (include/kanpyo_gpu.h, "word counts").  Any number of threads may add at once; most_common, info and reset take it alone."""

    def __init__(self, words: Words, table_slots=None, key_bytes=None):
        opts = _lib.CountsOpts(C.sizeof(_lib.CountsOpts), 0, int(table_slots or 0), int(key_bytes or 0))
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_counts_create(words.handle, C.byref(opts), C.byref(h)))
        self._h = h
        self.words = words

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().kgpu_counts_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_packed(self, utf8: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """kgpu_count_batch -> status[uint8 n].  KgpuError with KGPU_ERR_CAPACITY: some tokens found no room (info()["overflow_tokens"])."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        status = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(_lib.lib().kgpu_count_batch(self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, status.ctypes.data))
        return status[:n]

    def add(self, sentences: Sequence) -> np.ndarray:
        """The sentences (str or bytes) tokenized and counted -> their status bytes."""
        return self.add_packed(*pack_sentences(sentences))

    def add_text(self, block) -> np.ndarray:
        """kgpu_count_text: a raw block of input (bytes or uint8 array), split and trimmed on the device -> one status byte per line."""
        src = _block_bytes(block)
        cap = src.size // 16 + 1024
        L = _lib.lib()
        while True:
            status = np.zeros(cap, dtype=np.uint8)
            n = C.c_uint64(0)
            rc = L.kgpu_count_text(self._h, src.ctypes.data if src.size else None, src.size, status.ctypes.data, cap, C.byref(n))
            if rc == _lib.KGPU_ERR_CAPACITY and int(n.value) > cap:   # nothing was counted: the exact size, once more
                cap = int(n.value)
                continue
            _lib.check(rc)
            return status[: int(n.value)]

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
        return {n: int(getattr(i, n)) for n, _ in i._fields_ if n not in ("size", "reserved")}

    def reset(self):
        _lib.check(_lib.lib().kgpu_counts_reset(self._h))

    def vocabulary(self, max_size=None, min_count=1, specials=("<pad>", "<unk>"), unk="<unk>", bos=None, eos=None) -> "Vocab":
        """A Vocab chosen from these counts: specials + [w for w, c in most_common() if c >= min_count][:max_size - len(specials)], words equal
        to a special dropped from the tail.  unk, bos, eos: words of the list (put them among the specials) whose indices become unk_id, bos_id,
        eos_id; bos / eos None: not added.  Vocab.words keeps the list."""
        from .vocab import Vocab

        head = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in specials]
        taken = set(head)
        tail = [w for w, c in self.most_common() if c >= min_count and w not in taken]
        if max_size is not None:
            tail = tail[: max(int(max_size) - len(head), 0)]
        return Vocab.from_words(self.words, head + tail, unk, bos, eos)


def _block_bytes(block) -> np.ndarray:
    """A block of input (bytes-like or uint8 array) as a contiguous uint8 array."""
    return np.frombuffer(bytes(block), dtype=np.uint8) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block, dtype=np.uint8)


def split_lines(block) -> tuple:
    """kgpu_split_lines: the CLI's read_line + trim_end (src/bin/kanpyo.rs:114-122) over a block of input bytes
    -> (uint8 trimmed lines packed, uint64 offsets[n+1]).  Host only: needs no device."""
    src = _block_bytes(block)
    n_max = int(np.count_nonzero(src == 10)) + 1
    out = np.empty(max(src.size, 1), dtype=np.uint8)
    offs = np.empty(n_max + 1, dtype=np.uint64)
    n = C.c_uint64(0)
    _lib.check(_lib.lib().kgpu_split_lines(src.ctypes.data if src.size else None, src.size, out.ctypes.data, offs.ctypes.data, offs.size, C.byref(n)))
    k = int(n.value)
    return out[: int(offs[k])], offs[: k + 1]


def tokenize_packed_multi(tokenizers: Sequence[Tokenizer], utf8: np.ndarray, offsets: np.ndarray, token_capacity: int | None = None, out=None, compact: bool = False):
    """kgpu_tokenize_batch_multi: sentence i -> tokenizers[i mod G] (one Tokenizer per device; the same one may appear more than once), results in
    the caller's original order -- byte for byte what Tokenizer.tokenize_packed gives on one device.
    -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 n+1], status[uint8 n]).
    compact=True: kgpu_tokenize_batch_multi_compact -> (tokens8[TOKEN8_DTYPE], first[uint32 n x 2], tok_offsets, status); kanpyo_amd.device.expand_tokens
    (kgpu_expand_tokens) restores the 24-byte records where they are consumed."""
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    if n < 0:
        raise ValueError("offsets needs n+1 entries")
    total = int(offsets[-1] - offsets[0]) if n else 0
    cap = int(token_capacity) if token_capacity is not None else total // 2 + n + 64
    L = _lib.lib()
    handles = (C.c_void_p * len(tokenizers))(*[t.handle for t in tokenizers])
    first = np.zeros((max(n, 1), 2), dtype=np.uint32) if compact else None
    while True:
        if out is not None:
            tokens, toff, status = out
            cap = tokens.size
            token_capacity = cap
        else:
            tokens = np.empty(cap, dtype=TOKEN8_DTYPE if compact else TOKEN_DTYPE)
            toff = np.empty(n + 1, dtype=np.uint64)
            status = np.empty(max(n, 1), dtype=np.uint8)
        status[: max(n, 1)] = 0
        got = C.c_uint64(0)
        u = utf8.ctypes.data if utf8.size else None
        if compact:
            rc = L.kgpu_tokenize_batch_multi_compact(handles, len(tokenizers), u, offsets.ctypes.data, n, tokens.ctypes.data, cap, first.ctypes.data,
                                                     toff.ctypes.data, status.ctypes.data, C.byref(got))
        else:
            rc = L.kgpu_tokenize_batch_multi(handles, len(tokenizers), u, offsets.ctypes.data, n, tokens.ctypes.data, cap, toff.ctypes.data, status.ctypes.data, C.byref(got))
        if rc == _lib.KGPU_ERR_CAPACITY and token_capacity is None:
            cap = int(got.value) + 64
            continue
        _lib.check(rc)
        if compact:
            return tokens[: int(got.value)], first[:n], toff[: n + 1], status[:n]
        return tokens[: int(got.value)], toff[: n + 1], status[:n]


def concurrent_callers(tok: Tokenizer, utf8: np.ndarray, offsets: np.ndarray, threads: int, calls_per_thread: int, n_pattern=(1,), expect=None) -> dict:
    """Measurement / test helper (kgpu_debug_concurrent_callers, not part of the public header): `threads` native host threads call
    kgpu_tokenize_batch in a loop -- thread t with n_pattern[t % len] sentences per call -- walking round the corpus.  expect=(tokens, offsets)
    of the whole corpus (e.g. the oracle's): every call's records are compared, `mismatching_calls` counts the ones that differ."""
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    L = _lib.lib()
    f = L.kgpu_debug_concurrent_callers
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    pat = np.ascontiguousarray(n_pattern, dtype=np.int32)
    stats = np.zeros(8, dtype=np.float64)
    et = eo = None
    if expect is not None:
        et = np.ascontiguousarray(expect[0]); eo = np.ascontiguousarray(expect[1], dtype=np.uint64)
        assert et.dtype == TOKEN_DTYPE
    _lib.check(f(tok.handle, utf8.ctypes.data, offsets.ctypes.data, offsets.size - 1, int(threads), int(calls_per_thread), pat.ctypes.data, pat.size,
                 et.ctypes.data if et is not None else None, eo.ctypes.data if eo is not None else None, stats.ctypes.data))
    return {"wall_s": float(stats[0]), "p50_us": float(stats[1]), "p99_us": float(stats[2]), "mean_us": float(stats[3]), "mismatching_calls": int(stats[4]),
            "calls": int(stats[5]), "sentences": int(stats[6]), "sentences_per_s": float(stats[6] / stats[0]) if stats[0] > 0 else 0.0,
            "threads": int(threads), "n_pattern": [int(x) for x in pat], "caller_cpu_s": float(stats[7])}


TOKEN8_DTYPE = np.dtype([("id", "<i4"), ("packed", "<u4")])  # kgpu_token8


def merge_shards(shards, cnt: int, slice_sentences: int = 2048, reps: int = 1, token_capacity: int | None = None, want_tokens: bool = True, compact: bool = False):
    """Measurement / test helper (kgpu_debug_merge_shards[_compact], not part of the public header; needs NO device): the host-side merge of
    kgpu_tokenize_batch_multi[_compact] over one super-chunk of `cnt` sentences.  shards[g] = (rec[TOKEN8_DTYPE], first[uint32 m x 2], toff[uint64 m + 1],
    status[uint8 m]) as shard g's compaction kernel leaves them; sentence j of the super-chunk is shard j mod G's local sentence j // G.
    -> (rc, tokens, tok_offsets, status, n_tokens, seconds for all `reps` repetitions); compact: tokens = (tokens8, first[cnt x 2])."""
    G = len(shards)
    L = _lib.lib()
    vp = C.c_void_p
    keep = [[np.ascontiguousarray(a, dtype=dt) for a, dt in zip(sh, (TOKEN8_DTYPE, np.uint32, np.uint64, np.uint8))] for sh in shards]
    arr = lambda k: (vp * G)(*[sh[k].ctypes.data for sh in keep])
    total = sum(int(sh[2][-1]) for sh in keep)
    cap = total if token_capacity is None else int(token_capacity)
    tokens = np.zeros(max(cap, 1), dtype=TOKEN8_DTYPE if compact else TOKEN_DTYPE)
    toff = np.zeros(cnt + 1, dtype=np.uint64)
    status = np.full(max(cnt, 1), 255, dtype=np.uint8)
    n_tok, secs = C.c_uint64(0), C.c_double(0)
    if compact:
        f = L.kgpu_debug_merge_shards_compact
        f.argtypes = [C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_uint64, C.c_int, vp, vp, C.c_uint64, vp, vp,
                      C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        f.restype = C.c_int
        first = np.full((max(cnt, 1), 2), 0xABABABAB, dtype=np.uint32)
        rc = f(G, cnt, arr(0), arr(1), arr(2), arr(3), int(slice_sentences), int(reps), tokens.ctypes.data if want_tokens else None, first.ctypes.data, cap,
               toff.ctypes.data, status.ctypes.data, C.byref(n_tok), C.byref(secs))
        return rc, (tokens[: min(cap, total)], first[:cnt]), toff, status[:cnt], int(n_tok.value), float(secs.value)
    f = L.kgpu_debug_merge_shards
    f.argtypes = [C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_uint64, C.c_int, vp, C.c_uint64, vp, vp,
                  C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    f.restype = C.c_int
    rc = f(G, cnt, arr(0), arr(1), arr(2), arr(3), int(slice_sentences), int(reps), tokens.ctypes.data if want_tokens else None, cap, toff.ctypes.data,
           status.ctypes.data, C.byref(n_tok), C.byref(secs))
    return rc, tokens[: min(cap, total)], toff, status[:cnt], int(n_tok.value), float(secs.value)


def merge_bench(G: int = 8, sentences_per_shard: int = 8192, tokens_per_sentence: int = 32, reps: int = 20, compact: bool = False) -> dict:
    """The rate of that merge alone on this host's CPUs (bench.py's `multi_merge` entry): G synthetic shard blocks of a super-chunk, every sentence
    `tokens_per_sentence` records.  Per sentence the merge reads 8 t + 17 bytes and writes 24 t + 9 (t tokens): the 24-byte expansion is a
    memory-bandwidth job, so the rate is quoted beside a plain copy of the same number of bytes by the same worker threads' count of NumPy threads."""
    import time

    cnt = G * sentences_per_shard
    rng = np.random.default_rng(5)
    shards = []
    for g in range(G):
        m = sentences_per_shard
        toff = (np.arange(m + 1, dtype=np.uint64) * np.uint64(tokens_per_sentence))
        nt = int(toff[-1])
        rec = np.zeros(nt, dtype=TOKEN8_DTYPE)
        rec["id"] = rng.integers(1, 390000, size=nt)
        rec["packed"] = 1 | (2 << 2) | (6 << 14)
        shards.append((rec, np.zeros((m, 2), dtype=np.uint32), toff, np.zeros(m, dtype=np.uint8)))
    merge_shards(shards, cnt, reps=2, compact=compact)
    rc, _, _, _, n_tok, secs = merge_shards(shards, cnt, reps=reps, compact=compact)
    _lib.check(rc)
    moved = reps * ((n_tok * 16 + cnt * 34) if compact else (n_tok * 32 + cnt * 26))
    a = np.ones(n_tok * 24 // 8, dtype=np.uint64); b = np.empty_like(a)
    b[:] = a
    t0 = time.perf_counter()
    for _ in range(5):
        b[:] = a
    copy_gbs = 5 * a.nbytes * 2 / (time.perf_counter() - t0) / 1e9
    return {"sentences_per_s": reps * cnt / secs, "G": G, "sentences_per_super_chunk": cnt, "tokens_per_sentence": n_tok / cnt,
            "bytes_moved_GB_per_s": moved / secs / 1e9, "one_thread_copy_GB_per_s": copy_gbs, "record_bytes": 8 if compact else 24,
            "what": "kgpu_tokenize_batch_multi" + ("_compact" if compact else "") + "'s merge alone (no device): G shards' 8-byte records -> the caller's order as " + ("8" if compact else "24") + "-byte records + global offsets + "
                    "status bytes; slice totals from the shards' offset tables on the calling thread, one worker-pool task per 2048 sentences walks the G "
                    "cursors (no division per sentence); the calling thread's own share is O(slices x G)"}
