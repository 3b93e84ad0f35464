#!/usr/bin/env python
"""The N-best call's rate (kgpu_tokenize_batch_nbest, kgpu_nbest.hip) for k = 1, 5, 10 and 64, on the first 4096 sentences of the cfg 2 corpus and on
64 cfg 5 documents (the synthetic 392k dictionary).  No figure is a pass condition: nobody has measured any of this before.  The yardstick is the
lattice launch of the same run -- k_tokenize_general with BatchArgs::keep_lattice, which every chunk of the call pays whatever k is.

    python tools/nbest_rate.py [--out profiles/experiments/nbest_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  calls    per corpus and k the call's wall time (host memory in, host memory out; after a warm-up call at k = 64, which grows the arena) -> sentences/s.
  trace    per corpus measure.trace() over a child that makes the same calls, kernel tracing alone, in a run of its own: the time of
           k_tokenize_general beside k_nbest_forward and the three small kernels, per call, by k."""
import time

import measure

KS = (1, 5, 10, 64)
CALLS = 3
CORPORA = {"cfg2": 4096, "cfg5": 64}
KERNELS = ("k_tokenize_general", "k_nbest_forward", "k_nbest_count", "k_nbest_scan", "k_nbest_write")


def setup(kind):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, CORPORA[kind], 1, kind)
    return tok, sents, pack_sentences(sents)


def chunks_of(offs) -> int:
    """The chunks kgpu_tokenize_batch_nbest cuts this input into: at most 256 KiB and 1024 sentences each (kgpu_lattice_call.h over cut_chunk)."""
    o, n, done, chunks = offs.tolist(), len(offs) - 1, 0, 0
    while done < n:
        m = 0
        while done + m < n and m < 1024 and (m == 0 or o[done + m + 1] - o[done] <= 256 << 10):
            m += 1
        done, chunks = done + m, chunks + 1
    return chunks


def run_calls(tok, utf8, offs, timed=None):
    """The warm-up call, then CALLS calls per k, in the order of KS, each ONE call of the library (the buffers sized by the warm-up's result, which
    bounds the others) -> the last call's (paths, records) per k."""
    tokens, _, _, costs, _ = tok.tokenize_nbest_packed(utf8, offs, max(KS))
    room = dict(token_capacity=len(tokens), path_capacity=len(costs))
    sizes = {}
    for k in KS:
        for _ in range(CALLS):
            t0 = time.perf_counter()
            tokens, _, _, costs, _ = tok.tokenize_nbest_packed(utf8, offs, k, **room)
            if timed is not None:
                timed.setdefault(k, []).append(time.perf_counter() - t0)
        sizes[k] = (len(costs), len(tokens))
    return sizes


def leg_calls(say):
    say(f"# tools/nbest_rate.py: synthetic 392k dictionary; {CALLS} calls per k behind a warm-up call at k = {max(KS)}; library {measure.library_hash()}")
    for kind in CORPORA:
        tok, sents, (utf8, offs) = setup(kind)
        timed = {}
        sizes = run_calls(tok, utf8, offs, timed)
        say(f"{kind}: {len(sents)} sentences, {int(offs[-1])} bytes")
        for k in KS:
            m, spread = measure.summary(timed[k])
            say(f"  k = {k:<2}  {m * 1e3:9.2f} ms per call, spread {100 * spread:.0f} %  -> {len(sents) / m:10.0f} sentences/s; {sizes[k][0]} paths, {sizes[k][1]} records")
        tok.close()
    return True


def trace_child(kind):
    tok, _, (utf8, offs) = setup(kind)
    run_calls(tok, utf8, offs)
    print(chunks_of(offs))


def leg_trace(say):
    for kind in CORPORA:
        out, ds = measure.trace(__file__, ["--leg", "trace-" + kind], 330, stats=False)
        chunks = int(out.split()[-1])
        say(f"{kind}: kernel time per call in us, by k (rocprofv3 --kernel-trace, a run of its own; the warm-up call's dispatches left out)")
        say("  k    " + "".join(f"{name:>20}" for name in KERNELS))
        if any(len(ds.get(name, [])) < len(KS) * CALLS * chunks for name in KERNELS):   # (a timed call launches each kernel once per chunk)
            say(f"  fewer dispatches than {len(KS) * CALLS} calls of {chunks} chunks make: {[(name, len(ds.get(name, []))) for name in KERNELS]}")
            return False
        for i, k in enumerate(KS):
            line = f"  {k:<5}"
            for name in KERNELS:
                d = ds[name]
                tail = d[len(d) - (len(KS) - i) * CALLS * chunks : len(d) - (len(KS) - i - 1) * CALLS * chunks]   # counted from the end: the calls of k
                line += f"{sum(tail) / 1e3 / CALLS:20.1f}"
            say(line)
    return True


LEGS = {"calls": (leg_calls, 400), "trace": (leg_trace, 700)}


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, None, {"trace-" + kind: (lambda kind=kind: trace_child(kind)) for kind in CORPORA}, skip=("trace",) if args.no_trace else ())
