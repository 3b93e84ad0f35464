#!/usr/bin/env python3
"""tests/golden/fixture_align.json: the source alignment (include/kanpyo_gpu.h, "source alignment") of a few named lines, derived from Python's
unicodedata alone -- the segments of tools/gen_normalize_tables.py, each normalised by unicodedata.normalize and compared with itself -- and crafted
token records with the spans the header's rules 8 - 10 give them, one record for every branch of the rules.

    python tools/gen_align_fixture.py            # writes tests/golden/fixture_align.json
    python tools/gen_align_fixture.py --print    # ... to stdout instead (the regeneration test)

The build never runs this; tests/test_align_cpu.py compares the committed file with a fresh run whenever the running Python carries the Unicode
version the file names.  An edit is [out_pos, src_pos, out_char, src_char, out_len, src_len, out_chars, src_chars], a token and a span are
[position, byte_len, start, end].
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import unicodedata as U

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_normalize_tables as G  # noqa: E402

ROOT = G.ROOT


def edits_of(data: bytes, form: str):
    """-> (normalised bytes, status, edits): one edit per segment whose normalised bytes differ from its source bytes; none for a line left as it is."""
    out, status = G.normalize_line(data, form)
    if status:
        return out, status, []
    edits, op, sp, oc, sc = [], 0, 0, 0, 0
    for seg in G.segments(data.decode("utf-8"), form):
        norm = U.normalize(form, seg)
        s, n = seg.encode("utf-8"), norm.encode("utf-8")
        if s != n:
            edits.append([op, sp, oc, sc, len(n), len(s), len(norm), len(seg)])
        op, sp, oc, sc = op + len(n), sp + len(s), oc + len(norm), sc + len(seg)
    assert op == len(out)
    return out, 0, edits


def span_of(token, edits):
    """Rules 8 - 10 for one record."""
    pos, blen, start, end = token

    def behind(e, byte, chr_):
        return byte - (e[0] + e[4]) + e[1] + e[5], chr_ - (e[2] + e[6]) + e[3] + e[7]

    before = [e for e in edits if e[0] <= pos]
    if not before:
        sb, sc = pos, start
    elif pos < before[-1][0] + before[-1][4]:
        sb, sc = before[-1][1], before[-1][3]
    else:
        sb, sc = behind(before[-1], pos, start)
    if blen == 0:
        return [sb, 0, sc, sc + (end - start)]
    q = pos + blen
    before = [e for e in edits if e[0] < q]
    if not before:
        eb, ec = q, end
    elif q <= before[-1][0] + before[-1][4]:
        eb, ec = before[-1][1] + before[-1][5], before[-1][3] + before[-1][7]
    else:
        eb, ec = behind(before[-1], q, end)
    return [sb, eb - sb, sc, ec]


def char_tokens(norm: str, cuts):
    """The records of a tokenisation of `norm` cut before the characters `cuts` (ascending, inside the string), and the EOS dummy behind them."""
    bounds = [0] + list(cuts) + [len(norm)]
    toks = []
    for a, b in zip(bounds, bounds[1:]):
        toks.append([len(norm[:a].encode()), len(norm[a:b].encode()), a, b])
    toks.append([len(norm.encode()), 0, len(norm), len(norm) + 3])
    return toks


CASES = [   # (name, form, text): what pins the granularity of the edits
    ("hankaku_ga", "NFKC", "\uff8a\uff9d\uff76\uff9e\uff78"),   # one two-code-point edit among one-code-point edits
    ("kabushiki", "NFKC", "\u3231"),                             # 1 -> 3 characters
    ("ufdfa", "NFKC", "\ufdfa"),                                 # 3 -> 33 bytes
    ("jamo_l_v_t", "NFC", "\u1100\u1161\u11a8"),                 # 3 -> 1
    ("e_acute_decomposed", "NFC", "e\u0301"),
    ("e_acute_precomposed", "NFC", "\u00e9"),                    # no edit
    ("hangul_precomposed", "NFC", "\uac01"),                     # walked, byte-identical: no edit either
    ("reorder_only", "NFC", "a\u0323\u0301"),                    # decided from the bytes
    ("reorder_swapped", "NFC", "a\u0301\u0323"),
    ("empty", "NFKC", ""),
    ("clean", "NFKC", "\u6771\u4eacabc"),
    ("mixed", "NFKC", "x\uff21y\u3231z"),
    ("mixed_nfc", "NFC", "x\uff21y\u3231z"),                     # nothing changes under NFC
]
# (name, form, text, records): crafted records over x U+FF21 y U+3231 z -> "xAy(" U+682A ")z", one for every branch of rules 8 - 10
MIXED = "x\uff21y\u3231z"
SPAN_CASES = [
    ("start_inside_edit_end_at_edit_end", "NFKC", MIXED, [[4, 4, 4, 6]]),          # U+682A ")"
    ("start_at_edit_end", "NFKC", MIXED, [[8, 1, 6, 7]]),                          # "z"
    ("end_inside_edit", "NFKC", MIXED, [[2, 2, 2, 4]]),                            # "y("
    ("end_at_edit_end", "NFKC", MIXED, [[0, 2, 0, 2]]),                            # "xA"
    ("no_edit_before", "NFKC", MIXED, [[0, 1, 0, 1]]),                             # "x"
    ("eos_after_edit", "NFKC", MIXED, [[9, 0, 7, 10]]),
    ("first_token_not_at_zero", "NFKC", MIXED, [[1, 1, 1, 2], [2, 1, 2, 3]]),      # "A", "y": the chain dropped "x"
    ("three_tokens_one_source", "NFKC", "\u3231", char_tokens("(\u682a)", [1, 2])),
    ("whole_line", "NFKC", MIXED, char_tokens("xAy(\u682a)z", [])),
    ("every_char", "NFKC", MIXED, char_tokens("xAy(\u682a)z", [1, 2, 3, 4, 5, 6])),
    ("clean_line", "NFKC", "\u6771\u4eacabc", char_tokens("\u6771\u4eacabc", [2])),
    ("empty_line", "NFKC", "", char_tokens("", [])),
    ("hankaku", "NFKC", "\uff8a\uff9d\uff76\uff9e\uff78", char_tokens("\u30cf\u30f3\u30ac\u30af", [2, 3])),
]


def render() -> str:
    cases = []
    for name, form, text in CASES:
        out, status, edits = edits_of(text.encode("utf-8"), form)
        cases.append({"name": name, "form": form, "input": text.encode("utf-8").hex(), "output": out.hex(), "status": status, "edits": edits})
    span_cases = []
    for name, form, text, tokens in SPAN_CASES:
        _, _, edits = edits_of(text.encode("utf-8"), form)
        span_cases.append({"name": name, "form": form, "input": text.encode("utf-8").hex(), "edits": edits, "tokens": tokens,
                           "spans": [span_of(t, edits) for t in tokens]})
    doc = {"unicode": U.unidata_version, "cases": cases, "span_cases": span_cases}
    return json.dumps(doc, indent=1, ensure_ascii=True, separators=(",", ": ")).replace("[\n    ", "[").replace(",\n    ", ", ").replace("\n   ]", "]") + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--print", action="store_true", help="write to stdout instead of tests/golden/fixture_align.json")
    args = ap.parse_args(argv)
    text = render()
    if args.print:
        sys.stdout.write(text)
        return 0
    with open(os.path.join(ROOT, "tests", "golden", "fixture_align.json"), "w", encoding="ascii") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
