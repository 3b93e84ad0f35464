#!/usr/bin/env python
"""`kanpyo graphviz` for a batch: kgpu_graphviz_batch (lattices kept in HBM, rendered on the device) against the only way to the same text
without it -- a loop of kgpu_lattice_dump + kanpyo_amd.lattice.graphviz_for per sentence -- on the 512 smoke sentences (the 20k dictionary of
__graft_entry__.smoke with synth.feature_tables), full_state false.

    python tools/graphviz_rate.py [--out profiles/experiments/graphviz_device.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  calls    the device call (wall time per call, after a warm-up call) and the loop (wall time per pass), alternated in one process, and their
           documents compared.
  trace    measure.trace() over a child that runs the device call alone: the call's kernels, held against the calls leg's wall time per call."""
import time

import measure

CALLS = 5


def setup():
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, known, unk = measure.synthetic_tokenizer(20000, seed=11)
    sents = ["すもももももももものうち", ""] + synth.make_corpus(sd, 510, 1, "cfg2")
    return tok, DictFile(sd.dict, known, unk), sents, pack_sentences(sents)


def trace_child():
    tok, _, _, (utf8, offs) = setup()
    for _ in range(CALLS + 1):
        tok.graphviz_packed(utf8, offs)


def leg_calls(say):
    from kanpyo_amd.lattice import dump_lattice, graphviz_for

    tok, df, sents, (utf8, offs) = setup()
    say(f"# tools/graphviz_rate.py: {len(sents)} smoke sentences ({int(offs[-1])} bytes), full_state false, dpi 48; library {measure.library_hash()}")
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
    d, lo = measure.summary(dev_t)[0], measure.summary(loop_t)[0]
    say(f"documents identical to the loop's: {same}; {text.size} bytes of DOT ({text.size / len(sents):.0f} per sentence)")
    say(f"kgpu_graphviz_batch (one call, host memory in, text out): median {d * 1e3:.2f} ms  (calls: {', '.join(f'{x * 1e3:.2f}' for x in dev_t)})")
    say(f"loop of kgpu_lattice_dump + lattice.graphviz_for:          median {lo * 1e3:.0f} ms  (passes: {', '.join(f'{x * 1e3:.0f}' for x in loop_t)})")
    say(f"  -> the device call is {lo / d:.0f} x the loop; {len(sents) / d / 1e3:.0f} k against {len(sents) / lo / 1e3:.2f} k sentences/s")
    measure.carry(call_seconds=d)
    return same


def leg_trace(say):
    d = measure.carried()["call_seconds"]
    _, ks = measure.trace(__file__, ["--leg", "trace-child"], 300)
    mine = {k: v for k, v in ks.items() if k.startswith("k_gv_") or k == "k_tokenize_general"}
    total = sum(ns for _, ns in mine.values())
    say(f"kernels of {CALLS + 1} calls (rocprofv3 --kernel-trace --stats, a run of its own): {total / 1e3 / (CALLS + 1):.0f} us of kernel time per call")
    for k in sorted(mine, key=lambda k: -mine[k][1]):
        c, ns = mine[k]
        say(f"  {k:<20} {c} launches, {ns / 1e3 / c:9.1f} us each, {ns / total * 100:5.1f} %")
    top = max(mine, key=lambda k: mine[k][1])
    say(f"  -> {top} dominates the kernel time; kernel time is {total / (CALLS + 1) / 1e9 / d * 100:.0f} % of a call's wall time")
    return True


LEGS = {"calls": (leg_calls, 300), "trace": (leg_trace, 400)}


if __name__ == "__main__":   # (no header of the parent's: the calls leg says it, with the size of the corpus it has built)
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, None, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
