#!/usr/bin/env python3
"""tests/golden/fixture_pack.json: the model inputs (include/kanpyo_gpu.h, "model inputs") of a few hand-checkable samples, written by the plain-Python
reference tests/pack_ref.py: a single and a pair that fit, the three cases of rule 4 (and the side assignment), the three-window example of rule 5, a
sample without room between two with rows, the trims, a windowed single.

    python tools/gen_pack_fixture.py            # writes tests/golden/fixture_pack.json
    python tools/gen_pack_fixture.py --print    # ... to stdout instead (the regeneration test)

The build never runs this; tests/test_pack_cpu.py compares the committed file with a fresh run and with kgpu_pack_host.  Element k of a sequence of
sample i has the id 100 i + 10 + k (b: + 50), the span [k, 1, k, k + 1] and the token index k: a row can be read by eye."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pack_ref as P  # noqa: E402

CLS, SEP, PAD = 1, 2, 0

# name, options, [(La, Lb or None) per sample]: the lengths are the RAW ones, trims included
CASES = [
    ("single_fits", dict(max_length=6, strategy=P.ONLY_FIRST), [(2, None), (4, None), (0, None)]),
    ("pair_fits", dict(max_length=8, strategy=P.ONLY_SECOND), [(2, 3), (0, 0), (5, 0)]),
    ("longest_first_rule4_short_side_kept", dict(max_length=10, strategy=P.LONGEST_FIRST, windows=False), [(2, 9), (9, 2)]),
    ("longest_first_rule4_both_beyond_room", dict(max_length=10, strategy=P.LONGEST_FIRST, windows=False), [(9, 10), (8, 8)]),
    ("longest_first_rule4_short_side_past_half", dict(max_length=10, strategy=P.LONGEST_FIRST, windows=False), [(5, 6), (6, 5)]),
    ("longest_first_single", dict(max_length=5, strategy=P.LONGEST_FIRST, windows=False), [(7, None)]),
    ("only_second_three_windows_rule5", dict(max_length=10, stride=2, strategy=P.ONLY_SECOND), [(2, 10)]),
    ("only_second_no_windows", dict(max_length=10, stride=2, strategy=P.ONLY_SECOND, windows=False), [(2, 10)]),
    ("no_room_between_rows", dict(max_length=8, stride=1, strategy=P.ONLY_SECOND), [(1, 9), (5, 9), (4, 9), (1, 2)]),
    ("only_first_pair_windows", dict(max_length=9, stride=0, strategy=P.ONLY_FIRST), [(8, 3)]),
    ("only_first_single_windows", dict(max_length=6, stride=3, strategy=P.ONLY_FIRST), [(7, None)]),
    ("trims", dict(max_length=7, strategy=P.ONLY_SECOND, trim_front=1, trim_back=1), [(4, 5), (1, 2), (2, 12)]),
]


def build():
    cases = []
    for name, opts, samples in CASES:
        pair = samples[0][1] is not None
        ids, off_a, off_b = [], [0], [0]
        seqs = [(i, 0, la) for i, (la, _) in enumerate(samples)] + ([(i, 50, lb) for i, (_, lb) in enumerate(samples)] if pair else [])
        offs = [0]
        spans, tix = [], []
        for i, bias, ln in seqs:
            ids += [100 * i + 10 + bias + k for k in range(ln)]
            spans += [[k, 1, k, k + 1] for k in range(ln)]
            tix += list(range(ln))
            offs.append(len(ids))
        n = len(samples)
        off_a, off_b = offs[: n + 1], (offs[n:] if pair else None)
        full = dict(dict(stride=0, windows=True, trim_front=0, trim_back=0), **opts)
        ref = P.pack(ids, off_a, ids if pair else None, off_b, cls_id=CLS, sep_id=SEP, pad_id=PAD, spans_in=spans, tix_in=tix, **full)
        cases.append({"name": name, "opts": dict(full, strategy=P.STRATEGY_NAMES[full["strategy"]], cls_id=CLS, sep_id=SEP, pad_id=PAD),
                      "ids": ids, "off_a": off_a, "off_b": off_b, "spans_in": spans, "tix_in": tix,
                      "input_ids": ref["input_ids"], "token_type_ids": ref["token_type_ids"], "attention_mask": ref["attention_mask"],
                      "spans": [[list(s) for s in row] for row in ref["spans"]], "token_index": ref["token_index"],
                      "row_offsets": ref["row_offsets"], "status": ref["status"]})
    return {"about": "model inputs of hand-checkable samples, written by tests/pack_ref.py (tools/gen_pack_fixture.py)", "cases": cases}


def dumps(doc) -> str:
    """One array per line where it is a row: the file is meant to be read."""
    lines = ["{", f' "about": {json.dumps(doc["about"])},', ' "cases": [']
    for ci, c in enumerate(doc["cases"]):
        lines.append("  {")
        keys = list(c)
        for ki, k in enumerate(keys):
            v, end = c[k], "," if ki + 1 < len(keys) else ""
            if k in ("input_ids", "token_type_ids", "attention_mask", "spans", "token_index") and v:
                lines.append(f'   "{k}": [')
                lines += [f"    {json.dumps(row)}" + ("," if ri + 1 < len(v) else "") for ri, row in enumerate(v)]
                lines.append("   ]" + end)
            else:
                lines.append(f'   "{k}": {json.dumps(v)}{end}')
        lines.append("  }" + ("," if ci + 1 < len(doc["cases"]) else ""))
    lines += [" ]", "}"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--print", action="store_true", help="write to stdout, not to tests/golden/fixture_pack.json")
    args = ap.parse_args()
    text = dumps(build())
    if args.print:
        sys.stdout.write(text)
        return
    with open(os.path.join(ROOT, "tests", "golden", "fixture_pack.json"), "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
