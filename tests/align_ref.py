"""What the source-alignment tests share (include/kanpyo_gpu.h, "source alignment"): an independent reference for a line's edit records (the generator's
segments, each normalised by unicodedata), the header's rules 8 - 10 for one record in plain Python, random tokenisations of normalised strings, and the
library's host functions behind canaries."""
import ctypes as C
import unicodedata

import numpy as np

import normalize_ref as N
from kanpyo_amd._calls import EDIT_DTYPE, SPAN_DTYPE, TOKEN_DTYPE

EDIT_FIELDS = ("out_pos", "src_pos", "out_char", "src_char", "out_len", "src_len", "out_chars", "src_chars")
SPAN_FIELDS = ("position", "byte_len", "start", "end")


def ref_edits(data: bytes, form: str):
    """-> (bytes, status, edits as 8-tuples): per segment an edit iff normalize(seg).encode() != seg.encode(), positions by running sums."""
    out, status = N.GEN.normalize_line(data, form)
    if status:
        return out, status, []
    edits, op, sp, oc, sc = [], 0, 0, 0, 0
    for seg in N.GEN.segments(data.decode("utf-8"), form):
        norm = unicodedata.normalize(form, seg)
        s, n = seg.encode("utf-8"), norm.encode("utf-8")
        if s != n:
            edits.append((op, sp, oc, sc, len(n), len(s), len(norm), len(seg)))
        op, sp, oc, sc = op + len(n), sp + len(s), oc + len(norm), sc + len(seg)
    return out, 0, edits


def edit_tuples(edits: np.ndarray):
    return [tuple(int(e[f]) for f in EDIT_FIELDS) for e in edits]


def edit_array(tuples) -> np.ndarray:
    a = np.zeros(len(tuples), dtype=EDIT_DTYPE)
    for i, t in enumerate(tuples):
        a[i] = tuple(t)
    return a


def token_array(records) -> np.ndarray:
    """[position, byte_len, start, end] records -> TOKEN_DTYPE (class dummy where byte_len is 0)."""
    a = np.zeros(len(records), dtype=TOKEN_DTYPE)
    for i, (pos, blen, start, end) in enumerate(records):
        a[i] = (1 if blen else 0, 1 if blen else 0, pos, start, end, blen)
    return a


def span_lists(spans: np.ndarray):
    return [[int(s[f]) for f in SPAN_FIELDS] for s in spans]


def py_span(token, edits):
    """Rules 8 - 10 for one [position, byte_len, start, end] record over a line's edit 8-tuples."""
    pos, blen, start, end = token
    oend = lambda e: e[0] + e[4]   # noqa: E731
    behind = lambda e, b, c: (b - oend(e) + e[1] + e[5], c - (e[2] + e[6]) + e[3] + e[7])   # noqa: E731
    at = [e for e in edits if e[0] <= pos]
    sb, sc = (pos, start) if not at else (at[-1][1], at[-1][3]) if pos < oend(at[-1]) else behind(at[-1], pos, start)
    if blen == 0:
        return [sb, 0, sc, sc + end - start]
    q = pos + blen
    at = [e for e in edits if e[0] < q]
    eb, ec = (q, end) if not at else (at[-1][1] + at[-1][5], at[-1][3] + at[-1][7]) if q <= oend(at[-1]) else behind(at[-1], q, end)
    return [sb, eb - sb, sc, ec]


def random_tokens(rng, norm: str, drop_first: bool = False):
    """A tokenisation of `norm` cut at random character boundaries, the EOS dummy behind it -> [position, byte_len, start, end] records."""
    cuts = sorted({int(c) for c in rng.integers(1, max(len(norm), 2), size=int(rng.integers(0, 6))) if c < len(norm)})
    bounds = [0] + cuts + [len(norm)] if norm else [0, 0]
    recs = [[len(norm[:a].encode()), len(norm[a:b].encode()), a, b] for a, b in zip(bounds, bounds[1:]) if b > a]
    if drop_first and len(recs) > 1:
        recs = recs[1:]
    return recs + [[len(norm.encode()), 0, len(norm), len(norm) + 3]]


def host_aligned(data: bytes, form: str, capacity=None, edit_capacity=None):
    """kgpu_normalize_host_aligned behind 0xEE canaries -> (rc, bytes, size reported, status, edit tuples, edits reported)."""
    from kanpyo_amd import _lib

    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(data) * 11 if capacity is None else capacity
    ecap = len(data) if edit_capacity is None else edit_capacity
    out = np.full(cap + 8, 0xEE, dtype=np.uint8)
    ed = np.full((ecap + 1) * 24, 0xEE, dtype=np.uint8)
    got, ne, st = C.c_uint64(0), C.c_uint64(0), C.c_uint8(0xEE)
    rc = _lib.lib().kgpu_normalize_host_aligned(N.FORMS[form], src.ctypes.data if src.size else None, src.size, out.ctypes.data, cap, C.byref(got), C.byref(st),
                                                ed.ctypes.data, ecap, C.byref(ne))
    assert (out[cap:] == 0xEE).all() and (ed[ecap * 24:] == 0xEE).all(), "the host function wrote past a capacity"
    if rc != 0:
        assert (out == 0xEE).all() and (ed == 0xEE).all(), "a failed call wrote something"
        return rc, b"", int(got.value), int(st.value), [], int(ne.value)
    return rc, out[: got.value].tobytes(), int(got.value), int(st.value), edit_tuples(ed[: ne.value * 24].view(EDIT_DTYPE)), int(ne.value)


def host_lines_aligned(lines, form: str):
    """The host function over a list of lines -> (text, text_offsets, status, edits[EDIT_DTYPE], edit_offsets) as the aligned batch calls return them."""
    outs, sts, eds = [], [], []
    for ln in lines:
        rc, out, _, st, edits, _ = host_aligned(bytes(ln), form)
        assert rc == 0
        outs.append(out)
        sts.append(st)
        eds.append(edits)
    off, eoff = np.zeros(len(outs) + 1, dtype=np.uint64), np.zeros(len(outs) + 1, dtype=np.uint64)
    if outs:
        off[1:] = np.cumsum([len(o) for o in outs])
        eoff[1:] = np.cumsum([len(e) for e in eds])
    return np.frombuffer(b"".join(outs), dtype=np.uint8), off, np.array(sts, dtype=np.uint8), edit_array([e for es in eds for e in es]), eoff


def host_spans(tokens, tok_offsets, edits, edit_offsets) -> np.ndarray:
    from kanpyo_amd.tokenizer import source_spans_host

    return source_spans_host(tokens, tok_offsets, edits, edit_offsets)


# ---- what the sweeps share (tests/test_gpu_normalize_sweep.py) -------------------------------------------------------------------------------------
def expected_lines(lines, form: str, unchanged_has_none: bool = False):
    """ref_edits over a list of lines -> (text, text_offsets, status, edits[EDIT_DTYPE], edit_offsets) as the aligned batch calls return them: status 1 is
    the strict decoder's, status 4 the generator's, the text unicodedata's.  unchanged_has_none: a status-0 line that unicodedata leaves as it is has no
    edits, without a walk over its segments (for batches of many thousands of lines)."""
    outs, sts, eds = [], [], []
    for ln in lines:
        ln = bytes(ln)
        if unchanged_has_none:
            out, st = N.GEN.normalize_line(ln, form)
            edits = ref_edits(ln, form)[2] if st == 0 and out != ln else []
        else:
            out, st, edits = ref_edits(ln, form)
        outs.append(out)
        sts.append(st)
        eds.append(edits)
    off, eoff = np.zeros(len(outs) + 1, dtype=np.uint64), np.zeros(len(outs) + 1, dtype=np.uint64)
    if outs:
        off[1:] = np.cumsum([len(o) for o in outs])
        eoff[1:] = np.cumsum([len(e) for e in eds])
    return np.frombuffer(b"".join(outs), dtype=np.uint8), off, np.array(sts, dtype=np.uint8), edit_array([e for es in eds for e in es]), eoff


def edit_columns(**cols) -> np.ndarray:
    """Edit records from one numpy column per field of EDIT_FIELDS."""
    a = np.zeros(len(cols["out_pos"]), dtype=EDIT_DTYPE)
    for f in EDIT_FIELDS:
        a[f] = cols[f]
    return a


def differing_edit_lines(got, got_off, want, want_off) -> np.ndarray:
    """The lines whose edit records differ between two batches of equally many lines (a line with another number of records differs)."""
    g, w = got_off.astype(np.int64), want_off.astype(np.int64)
    glen, wlen = np.diff(g), np.diff(w)
    bad = glen != wlen
    if g[-1] > len(got) or w[-1] > len(want) or (glen < 0).any():
        return np.arange(len(wlen))
    same = np.repeat(~bad, wlen)
    idx = np.arange(int(w[0]), int(w[-1]))[same]
    shift = np.repeat(g[:-1] - w[:-1], wlen)[same]
    diff = idx[got[idx + shift] != want[idx]]
    bad[np.searchsorted(w, diff, side="right") - 1] = True
    return np.nonzero(bad)[0]


__all__ = ["EDIT_DTYPE", "SPAN_DTYPE", "TOKEN_DTYPE"]
