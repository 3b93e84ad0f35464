"""A plain reference for the ids with spans (include/kanpyo_gpu.h, "ids with spans"): rules 1 to 6 restated on Python lists.

Which tokens give ids and which word they have is encode_ref.sentence_words' walk (words_ref.row_word / row_dropped) with the record's index and four
fields kept; the pieces and where they end are wordpiece_ref.tables / char_starts; a span goes through a line's edits by align_ref.py_span.  encode()
asserts that its ids and offsets ARE encode_ref.encode's / wordpiece_ref.encode's, so this reference cannot drift from the two it stands on.  Nothing
comes from the library.  tests/test_encode_spans_cpu.py pins it against the hand-checkable tests/golden/fixture_encode_spans.json."""
import numpy as np

import align_ref as A
import encode_ref as E
import wordpiece_ref as WP
import words_ref as W

SPECIAL_SPAN, SPECIAL_INDEX = [0, 0, 0, 0], -1
M32 = 0xFFFFFFFF


def _bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def piece_ends(tabs, word, max_chars, unk_id):
    """wordpiece_ref.split_with that keeps where every piece ends -> (ids, [(byte end, character end)]).  The one id of a word that gives unk_id (rule 4b
    or 4d of "WordPiece ids") ends where the word ends."""
    initial, cont = tabs
    word = _bytes(word)
    if not word:
        return [], []
    starts = WP.char_starts(word)
    whole = ([unk_id], [(len(word), len(starts))])
    if len(starts) > max_chars:
        return whole
    bounds = starts[1:] + [len(word)]   # bounds[c - 1]: where the word's first c characters end
    ids, ends, start, c = [], [], 0, 0
    while start < len(word):
        table = initial if start == 0 else cont
        for ce in range(len(bounds), c, -1):   # the largest end first
            if word[start : bounds[ce - 1]] in table:
                ids.append(table[word[start : bounds[ce - 1]]])
                ends.append((bounds[ce - 1], ce))
                start, c = bounds[ce - 1], ce
                break
        else:
            return whole
    return ids, ends


def elements(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, wordpiece=False, prefix=b"##", max_chars=100, stats=None):
    """Rules 2 to 5 -> per sentence the list of (id, [position, byte_len, start, end], token index) its kept tokens give, no specials, no edits.
    stats: an optional dict that receives counts -- "row_split" / "text_split" (tokens that give their own pieces' spans, row-determined / keyed by
    the text), "whole_split" (several pieces, every one with the token's whole span), "unk", "dropped" -- and "max_records"."""
    raw = bytes(np.asarray(utf8, dtype=np.uint8).tobytes() if not isinstance(utf8, (bytes, bytearray)) else utf8)
    W.check_records(offsets, tokens, tok_offsets, n_known, n_unk)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    tokens = np.asarray(tokens)
    col = {f: tokens[f].tolist() for f in ("cls", "id", "position", "byte_len", "start", "end")}
    tabs = WP.tables(vocab, prefix) if wordpiece else None
    index = None if wordpiece else {_bytes(w): k for k, w in enumerate(vocab)}
    rows, splits = {}, {}
    no_row = (W.row_word(None, spec), W.row_dropped(None, spec))
    st = stats if stats is not None else {}
    for key in ("row_split", "text_split", "whole_split", "unk", "dropped", "max_records"):
        st.setdefault(key, 0)
    out = []
    for s in range(offsets.size - 1):
        base, k0 = int(offsets[s]), int(toff[s])
        st["max_records"] = max(st["max_records"], int(toff[s + 1]) - k0)
        sent = []
        for k in range(k0, int(toff[s + 1])):
            cls, tid = col["cls"][k], col["id"][k]
            if cls == W.DUMMY:
                continue
            if tid == 0:
                word, drop = no_row
            else:
                if (cls, tid) not in rows:
                    f = (known if cls == W.KNOWN else unk).features(tid)
                    rows[(cls, tid)] = (W.row_word(f, spec), W.row_dropped(f, spec))
                word, drop = rows[(cls, tid)]
            if drop:
                st["dropped"] += 1
                continue
            pos, blen = col["position"][k], col["byte_len"][k]
            whole = [pos, blen, col["start"][k], col["end"][k]]
            surface = word is None   # rule 4: the word is the text's -- for a known token the dictionary's key
            if surface:
                word = _bytes(keys[tid - 1]) if cls == W.KNOWN and tid != 0 else raw[base + pos : base + pos + blen]
            if not wordpiece:
                sent.append((index.get(word, unk_id), whole, k - k0))
                continue
            if word not in splits:
                splits[word] = piece_ends(tabs, word, max_chars, unk_id)
            ids, ends = splits[word]
            if len(ids) >= 2 and surface and len(word) == blen:   # rule 4: every piece its own bytes and characters of the token
                b = cb = 0
                for i, (e, ce) in zip(ids, ends):
                    sent.append((i, [(pos + b) & M32, e - b, (whole[2] + cb) & M32, (whole[2] + ce) & M32], k - k0))
                    b, cb = e, ce
                st["row_split" if cls == W.KNOWN and tid != 0 else "text_split"] += 1
            else:   # rule 5
                sent.extend((i, whole, k - k0) for i in ids)
                st["whole_split"] += len(ids) >= 2
                st["unk"] += len(ids) == 1 and word not in tabs[0]
        out.append(sent)
    return out


def encode(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, bos_id=None, eos_id=None, wordpiece=False, prefix=b"##",
           max_chars=100, edits=None, stats=None):
    """-> (ids int32, id_offsets uint64 [n + 1], spans uint32 [total, 4], token_index int32 [total]): rules 1 to 6.  edits: per sentence the list of its
    edit 8-tuples (align_ref.EDIT_FIELDS), or None for "no mapping"."""
    per = elements(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, wordpiece, prefix, max_chars, stats)
    ids, spans, index, off = [], [], [], [0]
    for s, sent in enumerate(per):
        if bos_id is not None:
            ids.append(bos_id); spans.append(SPECIAL_SPAN); index.append(SPECIAL_INDEX)
        for i, span, k in sent:
            ids.append(i)
            spans.append([v & M32 for v in (A.py_span(span, edits[s]) if edits is not None else span)])
            index.append(k)
        if eos_id is not None:
            ids.append(eos_id); spans.append(SPECIAL_SPAN); index.append(SPECIAL_INDEX)
        off.append(len(ids))
    ids, off = np.array(ids, dtype=np.int64).astype(np.int32), np.array(off, dtype=np.uint64)
    if wordpiece:
        old = WP.encode(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, bos_id, eos_id, prefix, max_chars)
    else:
        old = E.encode(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, keys, vocab, unk_id, bos_id, eos_id)
    assert np.array_equal(ids, old[0]) and np.array_equal(off, old[1]), "the span reference's ids are not the id reference's"
    return ids, off, np.array(spans, dtype=np.uint32).reshape(-1, 4), np.array(index, dtype=np.int32)


def padded(ids, id_offsets, spans, index, width, pad_id, eos_id=None):
    """The padded form from the ragged one -> (ids int32 [n, width], spans uint32 [n, width, 4], token_index int32 [n, width]): encode_ref.padded for the
    ids; the other two rows alike, with zeros and -1 in the pad slots and in the last slot of a cut row that ends with eos_id."""
    off = np.asarray(id_offsets).astype(np.int64)
    n = off.size - 1
    out_s, out_i = np.zeros((n, width, 4), dtype=np.uint32), np.full((n, width), SPECIAL_INDEX, dtype=np.int32)
    for s in range(n):
        m = min(int(off[s + 1] - off[s]), width)
        out_s[s, :m], out_i[s, :m] = spans[off[s] : off[s] + m], index[off[s] : off[s] + m]
        if off[s + 1] - off[s] > width and eos_id is not None:
            out_s[s, width - 1], out_i[s, width - 1] = 0, SPECIAL_INDEX
    return E.padded(ids, id_offsets, width, pad_id, eos_id), out_s, out_i
