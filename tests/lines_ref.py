"""A plain reference for the line renderer (kgpu_format.hip) and the generators of crafted records its tests share.

render() restates print_tokens (reference src/bin/kanpyo.rs:174-197) on bytes: per record the surface -- the record's byte_len bytes at
`position` of its sentence, the literal EOS for the dummy class -- then '\\t', the joined features of row id - 1 (nothing for the dummy class
and for id 0), then '\\n'.  It works on Python bytes and numpy only and imports nothing from the library's parser, pool or kernels;
tests/test_lines_ref_cpu.py pins it against the per-token loop of tests/test_gpu_lines.py (expected_lines, below) and the hand-derived fixture lines, so the expected
values of tests/test_gpu_format.py are themselves checked wherever the CPU suite runs."""
import numpy as np

# kgpu_token (include/kanpyo_gpu.h); tests/test_lines_ref_cpu.py holds it equal to kanpyo_amd.tokenizer.TOKEN_DTYPE
TOKEN_DTYPE = np.dtype([("id", "<i4"), ("cls", "<u4"), ("position", "<u4"), ("start", "<u4"), ("end", "<u4"), ("byte_len", "<u4")])
DUMMY, KNOWN, UNKNOWN = 0, 1, 2

KINDS = ("known", "known_edge", "unk", "unk_edge", "known0", "dummy", "dummy_id", "empty0", "emptyB", "overlap", "backwards")


def expected_lines(utf8, offs, tokens, tok_offsets, known, unk):
    """(text bytes, text offsets[n + 1]) the reference prints for these records: print_tokens (kanpyo.rs:174-197) restated."""
    cache = ({}, {})
    out, toff, size = [], [0], 0
    for i in range(len(offs) - 1):
        raw = utf8[int(offs[i]) : int(offs[i + 1])].tobytes()
        for t in tokens[int(tok_offsets[i]) : int(tok_offsets[i + 1])]:
            cls, tid, pos, bl = int(t["cls"]), int(t["id"]), int(t["position"]), int(t["byte_len"])
            surf = b"EOS" if cls == 0 else raw[pos : pos + bl]
            feats = b""
            if cls != 0 and tid != 0:
                c = cache[cls - 1]
                if tid not in c:
                    c[tid] = ",".join((known if cls == 1 else unk).features(tid)).encode()
                feats = c[tid]
            line = surf + b"\t" + feats + b"\n"
            out.append(line)
            size += len(line)
        toff.append(size)
    return b"".join(out), np.array(toff, dtype=np.uint64)


def rows_of(table, n):
    """The joined feature byte strings of a display table (anything with .features(id) -> list of str), row id - 1, ids 1..n."""
    return [",".join(table.features(i)).encode() for i in range(1, n + 1)]


def _ragged_copy(dst, dst_at, src, src_at, lens):
    """dst[dst_at[i] : dst_at[i] + lens[i]] = src[src_at[i] : src_at[i] + lens[i]] for every i."""
    lens = lens.astype(np.int64)
    total = int(lens.sum())
    if total == 0:
        return
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    dst[np.repeat(dst_at.astype(np.int64), lens) + within] = src[np.repeat(src_at.astype(np.int64), lens) + within]


def _fields(offsets, tokens, tok_offsets, known_rows, unk_rows):
    """Per record, in the order the sentences name them: (sentence index, surface length, feature row index or -1)."""
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    toff = np.asarray(tok_offsets, dtype=np.uint64).astype(np.int64)
    n = offsets.size - 1
    counts = np.diff(toff)
    if (counts < 0).any():
        raise ValueError("token offsets run backwards")
    rec = np.asarray(tokens)[int(toff[0]) : int(toff[n])] if n else np.asarray(tokens)[:0]
    sent = np.repeat(np.arange(n, dtype=np.int64), counts)
    cls, tid = rec["cls"].astype(np.int64), rec["id"].astype(np.int64)
    pos, bl = rec["position"].astype(np.int64), rec["byte_len"].astype(np.int64)
    B = (offsets[1:] - offsets[:-1])[sent]
    real = cls != DUMMY
    if (cls > UNKNOWN).any() or (real & ((pos > B) | (bl > B - pos))).any():
        raise ValueError("a record's class or surface is outside its sentence")
    nk, nu = len(known_rows), len(unk_rows)
    named = real & (tid != 0)
    if (named & ((tid < 0) | (tid > np.where(cls == KNOWN, nk, nu)))).any():
        raise ValueError("a record's id is outside its table")
    row = np.where(named, np.where(cls == KNOWN, 0, nk) + tid - 1, -1)
    sl = np.where(real, bl, 3)
    src_at = np.where(real, offsets[:-1][sent] + pos, -1)   # -1: the literal EOS
    return sent, counts, sl, src_at, row


def line_lengths(utf8, offsets, tokens, tok_offsets, known_rows, unk_rows):
    """The byte length of every record's line, in order (their running sum is where each line starts)."""
    _, _, sl, _, row = _fields(offsets, tokens, tok_offsets, known_rows, unk_rows)
    rl = np.array([len(r) for r in known_rows] + [len(r) for r in unk_rows] + [0], dtype=np.int64)   # (row -1: the trailing 0)
    return sl + rl[row] + 2


def render(utf8, offsets, tokens, tok_offsets, known_rows, unk_rows):
    """-> (text bytes, uint64 text offsets[n + 1]): the lines print_tokens writes for these records, sentence after sentence."""
    raw = bytes(np.asarray(utf8, dtype=np.uint8).tobytes() if not isinstance(utf8, (bytes, bytearray)) else utf8)
    sent, counts, sl, src_at, row = _fields(offsets, tokens, tok_offsets, known_rows, unk_rows)
    n = counts.size
    rows = list(known_rows) + list(unk_rows)
    rl = np.array([len(r) for r in rows] + [0], dtype=np.int64)
    ro = np.concatenate([[0], np.cumsum(rl)]).astype(np.int64)
    # one source array: the input, then "EOS", then the feature rows
    src = np.frombuffer(raw + b"EOS" + b"".join(rows), dtype=np.uint8)
    eos_at, rows_at = len(raw), len(raw) + 3
    fl = rl[row]
    length = sl + fl + 2
    start = np.cumsum(length) - length
    total = int(length.sum())
    out = np.empty(total, dtype=np.uint8)
    _ragged_copy(out, start, src, np.where(src_at < 0, eos_at, src_at), sl)
    out[start + sl] = 9
    _ragged_copy(out, start + sl + 1, src, rows_at + ro[row], fl)
    out[start + length - 1] = 10
    ends = np.concatenate([[0], np.cumsum(length)])
    text_off = ends[np.concatenate([[0], np.cumsum(counts)])] if n else np.zeros(1, dtype=np.int64)
    return out.tobytes(), text_off.astype(np.uint64)


# ---- crafted records ----------------------------------------------------------------------------------------------------------------------
def pack(sent_bytes, per_sentence):
    """Sentence byte strings and per sentence a list of (id, cls, position, byte_len) -> (utf8, offsets, tokens, tok_offsets)."""
    utf8 = np.frombuffer(b"".join(sent_bytes), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in sent_bytes])]).astype(np.uint64)
    tok_offsets = np.concatenate([[0], np.cumsum([len(r) for r in per_sentence])]).astype(np.uint64)
    flat = [r for rs in per_sentence for r in rs]
    tokens = np.zeros(len(flat), dtype=TOKEN_DTYPE)
    if flat:
        a = np.array(flat, dtype=np.int64)
        tokens["id"], tokens["cls"], tokens["position"], tokens["byte_len"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return utf8, offsets, tokens, tok_offsets


def make_records(rng, n_sent, tokens_per_sentence, kinds, n_known, n_unk, max_bytes=48, max_surface=12, known_ids=None):
    """A seeded batch of crafted records, every one valid by line_of's rules (kgpu_format.hip).

    tokens_per_sentence: a count, a (low, high) tuple drawn per sentence (high included), or one count per sentence.  Sentences have 0 to
    max_bytes random bytes (one in eight has none); a record of a 0-byte sentence has position 0 and byte_len 0 whatever its kind.
    kinds, drawn uniformly per record:
      known       id uniform in 1..n_known (or drawn from known_ids), a random surface of at most max_surface bytes
      known_edge  id 1 or n_known             unk       id uniform in 1..n_unk            unk_edge  id 1 or n_unk
      known0      a known record with id 0 (no features)
      dummy       the EOS class with id 0, anywhere in the sentence; position and byte_len are noise (the dummy's are never read)
      dummy_id    the EOS class with a non-zero id, negative and beyond the tables included
      empty0      byte_len 0 at position 0    emptyB    byte_len 0 at position B (the sentence's byte length)
      overlap     the whole sentence as the surface (it overlaps every neighbour)
      backwards   one byte at position B - 1 - (index in the sentence) % B: surfaces that descend
    start / end (character positions the renderer never reads) are noise.  -> (utf8, offsets, tokens, tok_offsets)"""
    kinds = list(kinds)
    assert kinds and all(k in KINDS for k in kinds)
    if isinstance(tokens_per_sentence, tuple):
        counts = rng.integers(tokens_per_sentence[0], tokens_per_sentence[1] + 1, size=n_sent)
    elif np.ndim(tokens_per_sentence) == 0:
        counts = np.full(n_sent, int(tokens_per_sentence), dtype=np.int64)
    else:
        counts = np.asarray(tokens_per_sentence, dtype=np.int64)
        assert counts.size == n_sent
    nbytes = rng.integers(0, max_bytes + 1, size=n_sent)
    nbytes[rng.integers(0, 8, size=n_sent) == 0] = 0
    offsets = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.uint64)
    utf8 = rng.integers(0, 256, size=int(offsets[-1]), dtype=np.uint8)
    tok_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    T = int(tok_offsets[-1])
    sent = np.repeat(np.arange(n_sent), counts)
    idx = np.arange(T) - np.repeat(tok_offsets[:-1].astype(np.int64), counts)   # index in the sentence
    B = nbytes[sent].astype(np.int64)
    kind = np.array(kinds)[rng.integers(0, len(kinds), size=T)] if T else np.array([], dtype="<U10")
    # the defaults: a known record with a random surface
    pos = (rng.random(T) * (B + 1)).astype(np.int64)
    bl = np.minimum((rng.random(T) * (max_surface + 1)).astype(np.int64), B - pos)
    cls = np.full(T, KNOWN, dtype=np.int64)
    pool = np.arange(1, n_known + 1) if known_ids is None else np.asarray(known_ids, dtype=np.int64)
    tid = pool[rng.integers(0, pool.size, size=T)] if T else np.zeros(0, dtype=np.int64)
    pick = rng.integers(0, 2, size=T)
    m = kind == "known_edge"; tid[m] = np.where(pick[m] == 0, 1, n_known)
    m = kind == "unk"; cls[m] = UNKNOWN; tid[m] = rng.integers(1, n_unk + 1, size=int(m.sum()))
    m = kind == "unk_edge"; cls[m] = UNKNOWN; tid[m] = np.where(pick[m] == 0, 1, n_unk)
    m = kind == "known0"; tid[m] = 0
    noise = rng.integers(0, 1 << 32, size=(T, 2))
    m = kind == "dummy"; cls[m] = DUMMY; tid[m] = 0; pos[m] = noise[m, 0]; bl[m] = noise[m, 1]
    m = kind == "dummy_id"; cls[m] = DUMMY; pos[m] = noise[m, 0]; bl[m] = noise[m, 1]
    wild = np.array([1, -1, n_known, n_known + 1, n_unk + 7, 0x7FFFFFFF, -0x80000000])
    tid[m] = wild[rng.integers(0, wild.size, size=int(m.sum()))]
    m = kind == "empty0"; pos[m] = 0; bl[m] = 0
    m = kind == "emptyB"; pos[m] = B[m]; bl[m] = 0
    m = kind == "overlap"; pos[m] = 0; bl[m] = B[m]
    m = (kind == "backwards") & (B > 0); pos[m] = B[m] - 1 - idx[m] % B[m]; bl[m] = 1
    m = (kind == "backwards") & (B == 0); pos[m] = 0; bl[m] = 0
    tokens = np.zeros(T, dtype=TOKEN_DTYPE)
    tokens["id"], tokens["cls"], tokens["position"], tokens["byte_len"] = tid, cls, pos, bl
    tokens["start"], tokens["end"] = rng.integers(0, 1 << 32, size=T), rng.integers(0, 1 << 32, size=T)
    return utf8, offsets, tokens, tok_offsets


# ---- the shapes of tests/test_gpu_format.py (the CPU test runs every one of them through render and the per-token loop) ---------------------
WINDOW_TOKENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000)
WINDOW_MIS = (0, 1, 9, 15)
MANY_N = (0, 1, 255, 256, 257, 1023, 1024, 1025, 32767, 32768, 32769, 70001)


def window_case(regime, T, big_id=3):
    """One sentence of T records (test 2).  regime 'two': every line is the two bytes of a known record with id 0 and no surface; 'cycle': line
    lengths cycle through 2..40 (id 0, surfaces of 0..38 bytes); 'big': a line of 10 203 bytes or more (the row of big_id and a surface of
    1..5 bytes) at every third record, two-byte lines between."""
    text = bytes((7 * i + 33) % 251 for i in range(64))
    k = np.arange(T)
    if regime == "two":
        recs = [(0, KNOWN, (i * 5) % 65, 0) for i in k]
    elif regime == "cycle":
        recs = [(0, KNOWN, (i * 3) % 26, (i + T) % 39) for i in k]
    else:
        assert regime == "big"
        recs = [(big_id, KNOWN, i % 59, 1 + i % 5) if i % 3 == 0 else (0, KNOWN, 64, 0) for i in k]
    return pack([text], [recs])


def many_case(rng, n, n_known, n_unk, kinds=KINDS, long_at=()):
    """n sentences of 0-3 short records, half of them without any (test 3); the sentences named by long_at get 200 records."""
    counts = np.array([0, 0, 0, 1, 2, 3])[rng.integers(0, 6, size=n)]
    for s in long_at:
        counts[s] = 200
    return make_records(rng, n, counts, kinds, n_known, n_unk)


def big_case(rng, counts, row_id=3):
    """The shape of the 4 GiB test: sentence s has 251 bytes of text and counts[s] known records naming row_id; record k of a sentence is the
    one byte at position k % 251, so neighbouring lines differ and a line displaced by whole lines is seen (251 is coprime to 16)."""
    counts = np.asarray(counts, dtype=np.int64)
    n = counts.size
    utf8 = rng.integers(0, 256, size=251 * n, dtype=np.uint8)
    offsets = (np.arange(n + 1) * 251).astype(np.uint64)
    tok_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    T = int(tok_offsets[-1])
    idx = np.arange(T) - np.repeat(tok_offsets[:-1].astype(np.int64), counts)
    tokens = np.zeros(T, dtype=TOKEN_DTYPE)
    tokens["id"], tokens["cls"], tokens["position"], tokens["byte_len"] = row_id, KNOWN, idx % 251, 1
    return utf8, offsets, tokens, tok_offsets
