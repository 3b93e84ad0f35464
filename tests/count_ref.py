"""A plain reference for the word counts (include/kanpyo_gpu.h, "word counts"): the header's rules restated on Python bytes and a Counter.

count() takes token records, the two display tables, a words_ref.Spec and the dictionary's known surfaces by id (synth.record_surfaces, or the
fixture's keywords), and gives a Counter keyed by the word's bytes; ordered() gives the read-out's order.  Word choice, the filter and the
record checks are words_ref's own (row_word, row_dropped, check_records); nothing comes from the library.  tests/test_count_cpu.py pins it
against the hand-derived tests/golden/fixture_counts.json and against a Counter over words_ref.render's lines."""
from collections import Counter

import numpy as np

import words_ref as W


def _bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def count(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, own_records=False, into=None, ids=None):
    """-> Counter {word bytes: count} of the kept tokens (rules 1-3).  keys[id - 1]: the dictionary's key of known id `id` (rule 2: the word of a
    known token with an id whose word is its surface).  own_records: the records are a tokenizer's own -- every such key is asserted to equal the
    record's bytes in the text.  into: a Counter to add to (accumulation).  ids: an optional dict that receives, per word, the set of (class, id) counted under it."""
    raw = bytes(np.asarray(utf8, dtype=np.uint8).tobytes() if not isinstance(utf8, (bytes, bytearray)) else utf8)
    W.check_records(offsets, tokens, tok_offsets, n_known, n_unk)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    tokens = np.asarray(tokens)
    cls_a, id_a = tokens["cls"].tolist(), tokens["id"].tolist()
    pos_a, bl_a = tokens["position"].tolist(), tokens["byte_len"].tolist()
    out = Counter() if into is None else into
    cache = {}
    no_row = (W.row_word(None, spec), W.row_dropped(None, spec))
    for s in range(offsets.size - 1):
        base = int(offsets[s])
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
                surface = raw[base + pos_a[k] : base + pos_a[k] + bl_a[k]]
                if cls == W.KNOWN and tid != 0:
                    word = _bytes(keys[tid - 1])
                    if own_records:
                        assert word == surface, (tid, word, surface)
                else:
                    word = surface
            out[word] += 1
            if ids is not None:
                ids.setdefault(word, set()).add((cls, tid))
    return out


def ordered(counter, top=None):
    """Rule 5: [(word bytes, count)] by count descending, then bytes ascending (Python's bytes order is memcmp's, a proper prefix first)."""
    items = sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))
    return items if top is None else items[:top]
