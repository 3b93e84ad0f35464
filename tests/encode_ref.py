"""A plain reference for the vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids"): the header's rules restated on Python bytes and a dict.

Word choice, the filter and the record checks are words_ref's own (row_word, row_dropped, check_records); a known token with an id whose word
is its surface is the dictionary's key of that id, as count_ref has it; the lookup is a Python dict; key_hash restates the table's hash.
Nothing comes from the library.  tests/test_encode_cpu.py pins it against the hand-derived tests/golden/fixture_encode.json."""
import numpy as np

import words_ref as W


def _bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def key_hash(b):
    """FNV-1a over the bytes, the length folded in, murmur3's finaliser: the byte-keyed table's hash."""
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    h ^= len(b) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def sentence_words(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, sources=None):
    """-> per sentence the list of its kept tokens' words (bytes), rules 1 and 2.  keys[id - 1]: the dictionary's key of known id `id`.
    sources: an optional dict that receives, per word, the set of (class, id) it was reached through."""
    raw = bytes(np.asarray(utf8, dtype=np.uint8).tobytes() if not isinstance(utf8, (bytes, bytearray)) else utf8)
    W.check_records(offsets, tokens, tok_offsets, n_known, n_unk)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    tokens = np.asarray(tokens)
    cls_a, id_a = tokens["cls"].tolist(), tokens["id"].tolist()
    pos_a, bl_a = tokens["position"].tolist(), tokens["byte_len"].tolist()
    cache = {}
    no_row = (W.row_word(None, spec), W.row_dropped(None, spec))
    out = []
    for s in range(offsets.size - 1):
        base = int(offsets[s])
        words = []
        for k in range(int(toff[s]), int(toff[s + 1])):
            cls = cls_a[k]
            if cls == W.DUMMY:
                continue
            tid = id_a[k]
            if tid == 0:
                word, drop = no_row
            else:
                key = (cls, tid)
                if key not in cache:
                    f = (known if cls == W.KNOWN else unk).features(tid)
                    cache[key] = (W.row_word(f, spec), W.row_dropped(f, spec))
                word, drop = cache[key]
            if drop:
                continue
            if word is None:
                word = _bytes(keys[tid - 1]) if cls == W.KNOWN and tid != 0 else raw[base + pos_a[k] : base + pos_a[k] + bl_a[k]]
            words.append(word)
            if sources is not None:
                sources.setdefault(word, set()).add((cls, tid))
        out.append(words)
    return out


def encode_words(per_sentence, vocab, unk_id, bos_id=None, eos_id=None):
    """Rules 3-5 over sentence_words' lists -> (ids int32, id_offsets uint64[n + 1]).  vocab: the list; the same bytes twice is a ValueError."""
    index = {}
    for k, w in enumerate(vocab):
        w = _bytes(w)
        if w in index:
            raise ValueError(f"words {index[w]} and {k} of the list are the same bytes")
        index[w] = k
    ids, off = [], [0]
    for words in per_sentence:
        if bos_id is not None:
            ids.append(bos_id)
        ids.extend(index.get(w, unk_id) for w in words)
        if eos_id is not None:
            ids.append(eos_id)
        off.append(len(ids))
    return np.array(ids, dtype=np.int64).astype(np.int32), np.array(off, dtype=np.uint64)


def encode(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, bos_id=None, eos_id=None):
    """-> (ids int32, id_offsets uint64[n + 1]) of a batch's records."""
    return encode_words(sentence_words(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys), vocab, unk_id, bos_id, eos_id)


def padded(ids, id_offsets, width, pad_id, eos_id=None):
    """Rule 6 from the ragged form -> int32 [n, width]: the first `width` elements, pad_id behind; a cut row ends with eos_id when EOS is added."""
    off = np.asarray(id_offsets).astype(np.int64)
    n = off.size - 1
    out = np.full((n, width), pad_id, dtype=np.int32)
    for s in range(n):
        seq = ids[off[s] : off[s + 1]]
        out[s, : min(len(seq), width)] = seq[:width]
        if len(seq) > width and eos_id is not None:
            out[s, width - 1] = eos_id
    return out


def row_ids(known, unk, n_known, n_unk, spec, keys, vocab, unk_id):
    """The handle's row table: per feature row (known rows, then unknown rows) the id of the row's word, unk_id when it is not listed, None for an
    unknown row whose word is the surface (not row-determined: its entry is never read)."""
    index = {_bytes(w): k for k, w in enumerate(vocab)}
    out = []
    for cls, table, n in ((W.KNOWN, known, n_known), (W.UNKNOWN, unk, n_unk)):
        for tid in range(1, n + 1):
            word = W.row_word(table.features(tid), spec)
            if word is None:
                word = _bytes(keys[tid - 1]) if cls == W.KNOWN else None
            out.append(None if word is None else index.get(word, unk_id))
    return out


def probe(slots, arena, word):
    """A Python probe of a byte-keyed table as the library lays it out -> (id or None, slots walked past the home slot).  slots: uint64 [n, 2]
    ({tag, id}), tag = hash << 32 | (arena entry / 8 + 1); arena entries are {u32 length, u32 hash, bytes}."""
    word = _bytes(word)
    n = len(slots)
    assert n & (n - 1) == 0
    h = key_hash(word)
    i = h & (n - 1)
    for step in range(n):
        tag = int(slots[i][0])
        if tag == 0:
            return None, step
        if tag >> 32 == h:
            at = ((tag & 0xFFFFFFFF) - 1) * 8
            length = int.from_bytes(arena[at : at + 4], "little")
            if length == len(word) and bytes(arena[at + 8 : at + 8 + length]) == word:
                return int(np.int32(np.uint32(int(slots[i][1]) & 0xFFFFFFFF))), step
        i = (i + 1) & (n - 1)
    return None, n
