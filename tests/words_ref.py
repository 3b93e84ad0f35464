"""A plain reference for the wakati output (include/kanpyo_gpu.h, "wakati-gaki"): the header's six rules restated on Python bytes.

render() takes token records, two display tables (anything with .features(id) -> list of str, as kanpyo_amd.dictfile.MorphFeatureTable) and
a Spec, and gives for every sentence exactly one line: the words of its kept tokens joined by the separator byte, then a newline.  It works
on Python bytes and numpy only and imports nothing from the library; tests/test_words_cpu.py pins it against the hand-derived lines of
tests/golden/fixture_words.json, and pins the library's per-row word table against row_word() / row_dropped()."""
import numpy as np

SURFACE = -1
ALL, DROP, KEEP = 0, 1, 2
DUMMY, KNOWN, UNKNOWN = 0, 1, 2


class Spec:
    """field: SURFACE or a feature index; filter: ALL / DROP / KEEP with `names` (str or bytes); sep: one byte."""

    def __init__(self, field=SURFACE, filter=ALL, names=(), sep=b" "):
        self.field, self.filter = int(field), int(filter)
        self.names = frozenset(n.encode() if isinstance(n, str) else bytes(n) for n in names)
        self.sep = sep.encode() if isinstance(sep, str) else bytes(sep)
        assert len(self.sep) == 1 and self.sep != b"\n" and self.field >= SURFACE and self.filter in (ALL, DROP, KEEP)

    def __repr__(self):
        return f"Spec(field={self.field}, filter={self.filter}, names={sorted(n.decode() for n in self.names)}, sep={self.sep!r})"


def row_word(features, spec):
    """Rule 2.  features: the row's feature strings, or None for a token without a row (id 0).  -> the word's bytes, or None: the surface."""
    if spec.field == SURFACE or features is None or len(features) <= spec.field:
        return None
    name = features[spec.field]
    if name == "" or name == "*":
        return None
    return name.encode()


def row_dropped(features, spec):
    """Rule 3.  A token without a row, or with an empty row, has no feature 0 and matches no name."""
    if spec.filter == ALL:
        return False
    match = bool(features) and features[0].encode() in spec.names
    return match if spec.filter == DROP else not match


def check_records(offsets, tokens, tok_offsets, n_known, n_unk):
    """Rule 6: ValueError for records the render rejects (class, id within its table, surface inside the sentence; the dummy class is exempt)."""
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    counts = np.diff(toff)
    if (counts < 0).any():
        raise ValueError("token offsets run backwards")
    n = offsets.size - 1
    rec = np.asarray(tokens)[int(toff[0]) : int(toff[n])] if n else np.asarray(tokens)[:0]
    sent = np.repeat(np.arange(n, dtype=np.int64), counts)
    cls, tid = rec["cls"].astype(np.int64), rec["id"].astype(np.int64)
    pos, bl = rec["position"].astype(np.int64), rec["byte_len"].astype(np.int64)
    B = (offsets[1:] - offsets[:-1])[sent]
    real = cls != DUMMY
    if (cls > UNKNOWN).any() or (real & ((pos > B) | (bl > B - pos))).any():
        raise ValueError("a record's class or surface is outside its sentence")
    if (real & (tid != 0) & ((tid < 0) | (tid > np.where(cls == KNOWN, n_known, n_unk)))).any():
        raise ValueError("a record's id is outside its table")


def render(utf8, offsets, tokens, tok_offsets, known, unk, n_known, n_unk, spec, counts=None):
    """-> (text bytes, uint64 text offsets[n + 1]).  counts: an optional dict that receives 'tokens' (non-EOS records) and 'dropped'."""
    raw = bytes(np.asarray(utf8, dtype=np.uint8).tobytes() if not isinstance(utf8, (bytes, bytearray)) else utf8)
    check_records(offsets, tokens, tok_offsets, n_known, n_unk)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    tokens = np.asarray(tokens)
    cls_a, id_a = tokens["cls"].tolist(), tokens["id"].tolist()
    pos_a, bl_a = tokens["position"].tolist(), tokens["byte_len"].tolist()
    cache = {}
    no_row = (row_word(None, spec), row_dropped(None, spec))
    out, text_off, size = [], [0], 0
    n_tok = n_drop = 0
    for s in range(offsets.size - 1):
        base = int(offsets[s])
        words = []
        for k in range(int(toff[s]), int(toff[s + 1])):
            cls = cls_a[k]
            if cls == DUMMY:   # rule 1: never a word, whatever its id, position and length
                continue
            n_tok += 1
            tid = id_a[k]
            if tid == 0:
                word, drop = no_row
            else:
                key = (cls, tid)
                if key not in cache:
                    f = (known if cls == KNOWN else unk).features(tid)
                    cache[key] = (row_word(f, spec), row_dropped(f, spec))
                word, drop = cache[key]
            if drop:
                n_drop += 1
                continue
            words.append(raw[base + pos_a[k] : base + pos_a[k] + bl_a[k]] if word is None else word)
        line = spec.sep.join(words) + b"\n"   # rules 4 and 5: nothing escaped; no words: the newline alone
        out.append(line)
        size += len(line)
        text_off.append(size)
    if counts is not None:
        counts["tokens"], counts["dropped"] = n_tok, n_drop
    return b"".join(out), np.array(text_off, dtype=np.uint64)
