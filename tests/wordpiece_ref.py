"""A plain reference for the WordPiece ids (include/kanpyo_gpu.h, "WordPiece ids"): the header's split rule restated on Python bytes and two dicts.

split() is BERT's WordpieceTokenizer on bytes: characters start at byte 0 and at every byte that is not 10xxxxxx; the piece at byte 0 is looked up in
the whole list, every later piece behind the prefix; the longest piece wins; a start with no piece makes the whole word unk_id.  Sentence-level
expectations stand on encode_ref.sentence_words (which tokens, which word) and encode_ref.padded.  Nothing comes from the library.
tests/test_wordpiece_cpu.py pins it against the hand-derived tests/golden/fixture_wordpiece.json and, where `tokenizers` is installed, against
tokenizers.models.WordPiece."""
import numpy as np

import encode_ref as E


def _bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def tables(vocab, prefix=b"##"):
    """-> (initial, continuation): bytes -> list index.  The same bytes twice in the list is a ValueError (vocabulary ids, rule 3)."""
    prefix = _bytes(prefix)
    initial = {}
    for k, w in enumerate(vocab):
        w = _bytes(w)
        if w in initial:
            raise ValueError(f"words {initial[w]} and {k} of the list are the same bytes")
        initial[w] = k
    if not prefix:
        return initial, initial
    return initial, {w[len(prefix):]: k for w, k in initial.items() if w.startswith(prefix) and len(w) > len(prefix)}


def char_starts(word):
    return [i for i in range(len(word)) if i == 0 or word[i] & 0xC0 != 0x80]


def split_with(tabs, word, max_chars, unk_id):
    initial, cont = tabs
    word = _bytes(word)
    if not word:
        return []
    starts = char_starts(word)
    if len(starts) > max_chars:
        return [unk_id]
    ends = set(starts[1:]) | {len(word)}
    out, start = [], 0
    while start < len(word):
        table = initial if start == 0 else cont
        for end in range(len(word), start, -1):
            if end in ends and word[start:end] in table:
                out.append(table[word[start:end]])
                start = end
                break
        else:
            return [unk_id]
    return out


def split(word, vocab, prefix=b"##", max_chars=100, unk_id=0):
    """The ids of one word's pieces."""
    return split_with(tables(vocab, prefix), word, max_chars, unk_id)


def encode_words(per_sentence, vocab, unk_id, bos_id=None, eos_id=None, prefix=b"##", max_chars=100, stats=None):
    """encode_ref.encode_words with every word's pieces in place of its one id -> (ids int32, id_offsets uint64[n + 1]).
    stats: an optional dict that receives the kept tokens by outcome: "whole" (one listed piece), "split", "unk", "empty"."""
    tabs = tables(vocab, prefix)
    cache = {}
    ids, off = [], [0]
    for words in per_sentence:
        if bos_id is not None:
            ids.append(bos_id)
        for w in words:
            if w not in cache:
                cache[w] = split_with(tabs, w, max_chars, unk_id)
            pieces = cache[w]
            ids.extend(pieces)
            if stats is not None:
                kind = "empty" if not pieces else "split" if len(pieces) > 1 else "whole" if w in tabs[0] else "unk"
                stats[kind] = stats.get(kind, 0) + 1
        if eos_id is not None:
            ids.append(eos_id)
        off.append(len(ids))
    return np.array(ids, dtype=np.int64).astype(np.int32), np.array(off, dtype=np.uint64)


def encode(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, bos_id=None, eos_id=None, prefix=b"##", max_chars=100, stats=None):
    """-> (ids int32, id_offsets uint64[n + 1]) of a batch's records."""
    words = E.sentence_words(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys)
    return encode_words(words, vocab, unk_id, bos_id, eos_id, prefix, max_chars, stats)


padded = E.padded


def rows(known, unk, n_known, n_unk, spec, keys, vocab, unk_id, prefix=b"##", max_chars=100):
    """The handle's row table: per feature row the list of its word's pieces; None for an unknown row whose word is the surface (never read)."""
    import words_ref as W

    tabs = tables(vocab, prefix)
    out = []
    for cls, table, n in ((W.KNOWN, known, n_known), (W.UNKNOWN, unk, n_unk)):
        for tid in range(1, n + 1):
            word = W.row_word(table.features(tid), spec)
            if word is None:
                word = _bytes(keys[tid - 1]) if cls == W.KNOWN else None
            out.append(None if word is None else split_with(tabs, word, max_chars, unk_id))
    return out


# ---- tests/golden/fixture_wordpiece.json: strings are UTF-8; {"hex": ...} is raw bytes; {"repeat": x, "times": n} is x n times ----------------
def golden_bytes(x):
    if isinstance(x, dict):
        if "hex" in x:
            return bytes.fromhex(x["hex"])
        return golden_bytes(x["repeat"]) * x["times"]
    return x.encode("utf-8")


def golden_pieces(pieces):
    """The expected pieces of a golden word as list entries (bytes), repeats expanded."""
    out = []
    for p in pieces:
        if isinstance(p, dict) and "repeat" in p:
            out += [golden_bytes(p["repeat"])] * p["times"]
        else:
            out.append(golden_bytes(p))
    return out
