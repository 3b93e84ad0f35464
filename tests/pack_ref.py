"""The model inputs (include/kanpyo_gpu.h, "model inputs") in plain Python: the reference of kgpu_pack_host and kgpu_pack_device.  Lists in, lists out;
written from the header's numbered rules, rule by rule, with no arithmetic shared with the library (rows are BUILT here, element by element, where the
library derives a slot's region)."""
from __future__ import annotations

import numpy as np

WINDOWS = 1
LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2
OK, CUT, NO_ROOM = 0, 1, 2
STRATEGY_NAMES = {LONGEST_FIRST: "longest_first", ONLY_FIRST: "only_first", ONLY_SECOND: "only_second"}
ZERO_SPAN = (0, 0, 0, 0)


class BadOffsets(ValueError):
    """rule 8"""


def trimmed(seq, trim_front, trim_back):
    """rule 1: a list of elements without its trims"""
    if len(seq) < trim_front + trim_back:
        return []
    return seq[trim_front : len(seq) - trim_back]


def slices_of(La, Lb, pair, max_length, stride, strategy, windows):
    """rules 3 to 5 -> (status, [(a_start, a_len, b_start, b_len) per row])"""
    room = max_length - (3 if pair else 2)
    if La + Lb <= room:
        return OK, [(0, La, 0, Lb)]
    if strategy == LONGEST_FIRST:
        if not pair:
            return CUT, [(0, room, 0, 0)]
        s1, s2 = min(La, Lb), max(La, Lb)
        s2 = s1 if s1 > room else max(s1, room - s1)
        if s1 + s2 > room:
            s1 = room // 2
            s2 = s1 + room % 2
        al, bl = (s1, s2) if La <= Lb else (s2, s1)
        return CUT, [(0, al, 0, bl)]
    cut_a = strategy == ONLY_FIRST
    fixed, L = (Lb, La) if cut_a else (La, Lb)
    w = room - fixed
    if w < 1 or (windows and stride >= w):
        return NO_ROOM, []
    starts = [0]
    if windows:
        while starts[-1] + w < L:   # the last window is the first one that reaches L
            starts.append(starts[-1] + (w - stride))
    rows = []
    for st in starts:
        ln = min(w, L - st)
        rows.append((st, ln, 0, Lb) if cut_a else (0, La, st, ln))
    return CUT, rows


def pack(ids_a, off_a, ids_b=None, off_b=None, *, max_length, stride=0, strategy=ONLY_SECOND, windows=True, cls_id=101, sep_id=102, pad_id=0,
         trim_front=0, trim_back=0, spans_in=None, tix_in=None):
    """-> dict of lists: input_ids, token_type_ids, attention_mask, spans, token_index (rows of max_length), row_offsets (n + 1), status (n).
    ids_a / ids_b: flat lists indexed by off_a / off_b (n + 1 entries each); off_b None: singles.  spans_in: a list of 4-tuples per id, tix_in: ints."""
    pair = off_b is not None
    n = len(off_a) - 1
    n_in = len(ids_a)
    out = {"input_ids": [], "token_type_ids": [], "attention_mask": [], "spans": [], "token_index": [], "row_offsets": [0], "status": []}
    for i in range(n):
        ranges = [(off_a[i], off_a[i + 1])] + ([(off_b[i], off_b[i + 1])] if pair else [])
        for lo, hi in ranges:
            if hi < lo or hi > n_in:
                raise BadOffsets(i)
        a = trimmed(list(range(off_a[i], off_a[i + 1])), trim_front, trim_back)   # element INDICES: ids, spans and token indices are looked up by them
        b = trimmed(list(range(off_b[i], off_b[i + 1])), trim_front, trim_back) if pair else []
        status, rows = slices_of(len(a), len(b), pair, max_length, stride, strategy, windows)
        out["status"].append(status)
        for a0, al, b0, bl in rows:
            src = [("cls", None)] + [("a", e) for e in a[a0 : a0 + al]] + [("sep", None)]
            types = [0] * (al + 2)
            if pair:
                src += [("b", e) for e in b[b0 : b0 + bl]] + [("sep", None)]
                types += [1] * (bl + 1)
            assert len(src) <= max_length, "a row longer than max_length"
            used = len(src)
            src += [("pad", None)] * (max_length - used)
            ids = [cls_id if k == "cls" else sep_id if k == "sep" else pad_id if k == "pad" else (ids_a if k == "a" else ids_b)[e] for k, e in src]
            out["input_ids"].append(ids)
            out["token_type_ids"].append(types + [0] * (max_length - used))
            out["attention_mask"].append([1] * used + [0] * (max_length - used))
            out["spans"].append([tuple(spans_in[e]) if e is not None and spans_in is not None else ZERO_SPAN for _, e in src])
            out["token_index"].append([tix_in[e] if e is not None and tix_in is not None else -1 for _, e in src])
        out["row_offsets"].append(len(out["input_ids"]))
    return out


def as_arrays(ref, max_length):
    """pack()'s lists as the arrays pack_host returns"""
    R = len(ref["input_ids"])
    rows = lambda k: np.array(ref[k], dtype=np.int32).reshape(R, max_length)   # noqa: E731
    return {"input_ids": rows("input_ids"), "token_type_ids": rows("token_type_ids"), "attention_mask": rows("attention_mask"), "token_index": rows("token_index"),
            "spans": np.array(ref["spans"], dtype=np.uint32).reshape(R, max_length, 4), "row_offsets": np.array(ref["row_offsets"], dtype=np.uint64),
            "status": np.array(ref["status"], dtype=np.uint8)}
