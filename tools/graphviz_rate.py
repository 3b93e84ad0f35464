#!/usr/bin/env python
"""`kanpyo graphviz` for a batch: kgpu_graphviz_batch (lattices kept in HBM, rendered on the device) against the only way to the same text
without it -- a loop of kgpu_lattice_dump + kanpyo_amd.lattice.graphviz_for per sentence -- on the 512 smoke sentences (the 20k dictionary of
__graft_entry__.smoke with synth.feature_tables), full_state false.

    python tools/graphviz_rate.py [--out profiles/experiments/graphviz_device.txt] [--no-trace]

Legs: the device call (wall time per call, after a warm-up call), the loop (wall time per pass), both alternated in one process and their
documents compared; the call's kernels under rocprofv3 --kernel-trace --stats (a child process running the device call alone)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CALLS = 5


def setup():
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.dictfile import DictFile
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict(20000, seed=11)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    sents = ["すもももももももものうち", ""] + synth.make_corpus(sd, 510, 1, "cfg2")
    return tok, DictFile(sd.dict, known, unk), sents, pack_sentences(sents)


def trace_leg(tmp):
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
           sys.executable, os.path.abspath(__file__), "--device-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
    out = {}
    with open(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"].split("(")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    tok, df, sents, (utf8, offs) = setup()
    if args.device_only:
        for _ in range(CALLS + 1):
            tok.graphviz_packed(utf8, offs)
        return
    from kanpyo_amd import _lib
    from kanpyo_amd.lattice import dump_lattice, graphviz_for

    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731
    say(f"# tools/graphviz_rate.py: {len(sents)} smoke sentences ({int(offs[-1])} bytes), full_state false, dpi 48; library {_lib.kernel_source_hash()}")
    text, toff, status = tok.graphviz_packed(utf8, offs)   # warm-up: contexts, arena, label pool
    dev_t, loop_t, same = [], [], True
    for _ in range(3):
        for _ in range(CALLS):
            t0 = time.perf_counter()
            text, toff, status = tok.graphviz_packed(utf8, offs)
            dev_t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        docs = [graphviz_for(dump_lattice(tok, s), df, 48, False) for s in sents]
        loop_t.append(time.perf_counter() - t0)
        same = same and "".join(docs).encode() == text.tobytes() and not status.any()
    d, lo = float(np.median(dev_t)), float(np.median(loop_t))
    say(f"documents identical to the loop's: {same}; {text.size} bytes of DOT ({text.size / len(sents):.0f} per sentence)")
    say(f"kgpu_graphviz_batch (one call, host memory in, text out): median {d * 1e3:.2f} ms  (calls: {', '.join(f'{x * 1e3:.2f}' for x in dev_t)})")
    say(f"loop of kgpu_lattice_dump + lattice.graphviz_for:          median {lo * 1e3:.0f} ms  (passes: {', '.join(f'{x * 1e3:.0f}' for x in loop_t)})")
    say(f"  -> the device call is {lo / d:.0f} x the loop; {len(sents) / d / 1e3:.0f} k against {len(sents) / lo / 1e3:.2f} k sentences/s")
    if not args.no_trace:
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            ks = trace_leg(tmp)
        mine = {k: v for k, v in ks.items() if k.startswith("k_gv_") or k == "k_tokenize_general"}
        total = sum(ns for _, ns in mine.values())
        say(f"kernels of {CALLS + 1} calls (rocprofv3 --kernel-trace --stats, a run of its own): {total / 1e3 / (CALLS + 1):.0f} us of kernel time per call")
        for k in sorted(mine, key=lambda k: -mine[k][1]):
            c, ns = mine[k]
            say(f"  {k:<20} {c} launches, {ns / 1e3 / c:9.1f} us each, {ns / total * 100:5.1f} %")
        top = max(mine, key=lambda k: mine[k][1])
        say(f"  -> {top} dominates the kernel time; kernel time is {total / (CALLS + 1) / 1e9 / d * 100:.0f} % of a call's wall time")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
