#!/usr/bin/env python
"""The lattice-probability calls' rate (kgpu_tokenize_batch_marginals, kgpu_tokenize_batch_samples, kgpu_prob.hip): the marginals of tokenize's path, and
samples at n_samples = 1, 8 and 64, on the first 4096 sentences of the cfg 2 corpus and on 64 cfg 5 documents (the synthetic 392k dictionary).  No figure
is a pass condition.  The yardstick is the lattice launch of the same run -- k_tokenize_general with BatchArgs::keep_lattice, which every chunk of a
call pays whatever it asks for; tools/nbest_rate.py's k = 1 row is what the forward kernel stands beside.

    python tools/prob_rate.py [--out profiles/experiments/prob_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  calls    per corpus and mode the call's wall time (host memory in, host memory out; after one warm-up call of the marginals and one of 64 samples, which
           grow the arena) -> sentences/s.
  trace    per corpus measure.trace() over a child that makes the same calls, kernel tracing alone, in a run of its own: the time of
           k_tokenize_general beside k_prob_forward, k_prob_backward and k_prob_sample (and the small kernels together), per call, by mode."""
import time

import measure

MODES = ("marginals", 1, 8, 64)   # the marginals call, then the samples call at these n_samples
CALLS = 3
CORPORA = {"cfg2": 4096, "cfg5": 64}
SMALL_M, SMALL_S = ("k_prob_count", "k_prob_scan", "k_prob_write"), ("k_prob_scan_paths", "k_prob_write_paths")
# kernel -> the modes whose calls launch it
USED_BY = {"k_tokenize_general": MODES, "k_prob_forward": MODES, "k_prob_backward": MODES[:1], "k_prob_sample": MODES[1:],
           **{k: MODES[:1] for k in SMALL_M}, **{k: MODES[1:] for k in SMALL_S}}
COLUMNS = ("k_tokenize_general", "k_prob_forward", "k_prob_backward", "k_prob_sample")


def setup(kind):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, CORPORA[kind], 1, kind)
    return tok, sents, pack_sentences(sents)


def chunks_of(offs) -> int:
    """The chunks the calls cut this input into: at most 256 KiB and 1024 sentences each (kgpu_lattice_call.h over cut_chunk)."""
    o, n, done, chunks = offs.tolist(), len(offs) - 1, 0, 0
    while done < n:
        m = 0
        while done + m < n and m < 1024 and (m == 0 or o[done + m + 1] - o[done] <= 256 << 10):
            m += 1
        done, chunks = done + m, chunks + 1
    return chunks


def run_calls(tok, utf8, offs, timed=None):
    """The two warm-up calls, then CALLS calls per mode, in the order of MODES, each ONE call of the library (the buffers sized by the warm-ups' results,
    which bound the others) -> the last call's (paths, records) per mode."""
    room_m = dict(token_capacity=len(tok.tokenize_marginals_packed(utf8, offs)[0]))
    tokens, _, _, costs, _ = tok.tokenize_samples_packed(utf8, offs, max(MODES[1:]), seed=1)   # (the same seed: sample i is the same path at every n_samples, so this call's sizes bound the others')
    room_s = dict(token_capacity=len(tokens), path_capacity=len(costs))
    sizes = {}
    for mode in MODES:
        for _ in range(CALLS):
            t0 = time.perf_counter()
            if mode == "marginals":
                got = tok.tokenize_marginals_packed(utf8, offs, **room_m)
                size = (len(offs) - 1, len(got[0]))
            else:
                got = tok.tokenize_samples_packed(utf8, offs, mode, seed=1, **room_s)
                size = (len(got[3]), len(got[0]))
            if timed is not None:
                timed.setdefault(mode, []).append(time.perf_counter() - t0)
        sizes[mode] = size
    return sizes


def label(mode) -> str:
    return "marginals   " if mode == "marginals" else f"samples {mode:<4}"


def leg_calls(say):
    say(f"# tools/prob_rate.py: synthetic 392k dictionary; theta = 0.75 / 800; {CALLS} calls per mode behind two warm-up calls; library {measure.library_hash()}")
    for kind in CORPORA:
        tok, sents, (utf8, offs) = setup(kind)
        timed = {}
        sizes = run_calls(tok, utf8, offs, timed)
        say(f"{kind}: {len(sents)} sentences, {int(offs[-1])} bytes")
        for mode in MODES:
            m, spread = measure.summary(timed[mode])
            say(f"  {label(mode)}  {m * 1e3:9.2f} ms per call, spread {100 * spread:.0f} %  -> {len(sents) / m:10.0f} sentences/s; {sizes[mode][0]} paths, {sizes[mode][1]} records")
        tok.close()
    return True


def trace_child(kind):
    tok, _, (utf8, offs) = setup(kind)
    run_calls(tok, utf8, offs)
    print(chunks_of(offs))


def calls_of(d, name, mode, chunks):
    """The dispatches of kernel `name` that the timed calls of `mode` made: counted from the end (the warm-up calls' dispatches come first and are left out)."""
    users = USED_BY[name]
    if mode not in users:
        return None
    behind = len(users) - users.index(mode)
    return d[len(d) - behind * CALLS * chunks : len(d) - (behind - 1) * CALLS * chunks]


def leg_trace(say):
    for kind in CORPORA:
        out, ds = measure.trace(__file__, ["--leg", "trace-" + kind], 330, stats=False)
        chunks = int(out.split()[-1])
        say(f"{kind}: kernel time per call in us, by mode (rocprofv3 --kernel-trace, a run of its own; the warm-up calls' dispatches left out)")
        say("  mode         " + "".join(f"{name:>20}" for name in COLUMNS) + f"{'count/scan/write':>20}")
        if any(len(ds.get(name, [])) < len(users) * CALLS * chunks for name, users in USED_BY.items()):   # (a timed call launches each of its kernels once per chunk)
            say(f"  fewer dispatches than {CALLS} calls of {chunks} chunks per mode make: {[(name, len(ds.get(name, []))) for name in USED_BY]}")
            return False
        for mode in MODES:
            line = f"  {label(mode)} "
            for name in COLUMNS:
                tail = calls_of(ds[name], name, mode, chunks)
                line += f"{'-':>20}" if tail is None else f"{sum(tail) / 1e3 / CALLS:20.1f}"
            small = sum(sum(calls_of(ds[name], name, mode, chunks)) for name in (SMALL_M if mode == "marginals" else SMALL_S))
            say(line + f"{small / 1e3 / CALLS:20.1f}")
    return True


LEGS = {"calls": (leg_calls, 400), "trace": (leg_trace, 700)}


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, None, {"trace-" + kind: (lambda kind=kind: trace_child(kind)) for kind in CORPORA}, skip=("trace",) if args.no_trace else ())
