#!/usr/bin/env python
"""The search / extended mode call's rate (kgpu_tokenize_batch_mode, kgpu_mode.hip) on the first 4096 sentences of the cfg 2 corpus (the synthetic
392k dictionary), one chunk of 1024 after the other.  The yardsticks come from the same run: the lattice launch -- k_tokenize_general with
BatchArgs::keep_lattice, which every chunk of the call pays in every mode -- and k_nbest_forward at k = 1, the kernel whose loads k_mode_forward
repeats with one wavefront minimum where that kernel sorts.

    python tools/mode_rate.py [--out profiles/experiments/mode_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  calls    per mode the call's wall time (host memory in, host memory out; after a warm-up call, which grows the arena) -> sentences/s, and the N-best
           call at k = 1 beside them.
  trace    measure.trace() over a child that makes the same calls, kernel tracing alone, in a run of its own: per call the time of k_tokenize_general,
           of k_nbest_forward (k = 1) and of k_mode_forward and the three small kernels by mode, each with its spread over the calls.  The leg is
           met when k_mode_forward in every mode takes no longer than k_nbest_forward at k = 1 plus the two kernels' spread in this run."""
import time

import measure

MODES = ("normal", "search", "extended")
CALLS = 5
SENTENCES = 4096
SMALL = ("k_mode_count", "k_mode_scan", "k_mode_write")


def setup():
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, SENTENCES, 1, "cfg2")
    return tok, sents, pack_sentences(sents)


def chunks_of(offs) -> int:
    """The chunks the call cuts this input into: at most 256 KiB and 1024 sentences each (kgpu_lattice_call.h over cut_chunk)."""
    o, n, done, chunks = offs.tolist(), len(offs) - 1, 0, 0
    while done < n:
        m = 0
        while done + m < n and m < 1024 and (m == 0 or o[done + m + 1] - o[done] <= 256 << 10):
            m += 1
        done, chunks = done + m, chunks + 1
    return chunks


def run_calls(tok, utf8, offs, timed=None):
    """A warm-up call of either kind, then CALLS calls of the N-best call at k = 1 and CALLS per mode, in the order of MODES, each ONE call of the
    library -> the last call's records per arm."""
    tokens, _, _, costs, _ = tok.tokenize_nbest_packed(utf8, offs, 1)
    room = dict(token_capacity=len(tokens), path_capacity=len(costs))
    wide = len(tok.tokenize_mode_packed(utf8, offs, "extended")[0])
    sizes = {}
    for arm in ("nbest k = 1",) + MODES:
        for _ in range(CALLS):
            t0 = time.perf_counter()
            got = tok.tokenize_nbest_packed(utf8, offs, 1, **room) if arm not in MODES else tok.tokenize_mode_packed(utf8, offs, arm, token_capacity=wide)
            if timed is not None:
                timed.setdefault(arm, []).append(time.perf_counter() - t0)
        sizes[arm] = len(got[0])
    return sizes


def leg_calls(say):
    say(f"# tools/mode_rate.py: synthetic 392k dictionary; {CALLS} calls per arm behind a warm-up call; library {measure.library_hash()}")
    tok, sents, (utf8, offs) = setup()
    timed = {}
    sizes = run_calls(tok, utf8, offs, timed)
    say(f"cfg2: {len(sents)} sentences, {int(offs[-1])} bytes, {chunks_of(offs)} chunks")
    for arm in timed:
        m, spread = measure.summary(timed[arm])
        say(f"  {arm:<12} {m * 1e3:9.2f} ms per call, spread {100 * spread:.0f} %  -> {len(sents) / m:10.0f} sentences/s; {sizes[arm]} records")
    tok.close()
    return True


def trace_child():
    tok, _, (utf8, offs) = setup()
    run_calls(tok, utf8, offs)
    print(chunks_of(offs))


def leg_trace(say):
    out, ds = measure.trace(__file__, ["--leg", "trace-child"], 330, stats=False)
    chunks = int(out.split()[-1])
    per = CALLS * chunks
    need = {"k_nbest_forward": per, "k_mode_forward": len(MODES) * per, **{name: len(MODES) * per for name in SMALL}, "k_tokenize_general": (1 + len(MODES)) * per}
    if any(len(ds.get(name, [])) < c for name, c in need.items()):
        say(f"  fewer dispatches than {CALLS} calls of {chunks} chunks make: {[(name, len(ds.get(name, []))) for name in need]}")
        return False

    def calls_of(name, i, arms):
        """Per call the kernel's time in us: the dispatches of arm i of `arms` timed arms, counted from the end (the warm-up calls' left out)."""
        d = ds[name]
        tail = d[len(d) - (arms - i) * per : len(d) - (arms - i - 1) * per]
        return [sum(tail[c * chunks : (c + 1) * chunks]) / 1e3 for c in range(CALLS)]

    say(f"cfg2: kernel time per call of {chunks} chunks in us, median and spread over {CALLS} calls (rocprofv3 --kernel-trace, a run of its own)")
    lattice = [measure.summary(calls_of("k_tokenize_general", i, 1 + len(MODES))) for i in range(1 + len(MODES))]
    nb, nb_spread = measure.summary(calls_of("k_nbest_forward", 0, 1))
    say(f"  {'nbest k = 1':<12} k_tokenize_general {lattice[0][0]:9.1f} ({100 * lattice[0][1]:.0f} %)   k_nbest_forward {nb:9.1f} ({100 * nb_spread:.0f} %)")
    met = True
    for i, mode in enumerate(MODES):
        fw, fw_spread = measure.summary(calls_of("k_mode_forward", i, len(MODES)))
        small = sum(measure.summary(calls_of(name, i, len(MODES)))[0] for name in SMALL)
        ok = fw <= nb * (1 + nb_spread + fw_spread)
        met = met and ok
        say(f"  {mode:<12} k_tokenize_general {lattice[1 + i][0]:9.1f} ({100 * lattice[1 + i][1]:.0f} %)   k_mode_forward  {fw:9.1f} ({100 * fw_spread:.0f} %)   count + scan + write {small:7.1f}"
            f"   forward / k_nbest_forward = {fw / nb:.2f}{'' if ok else '  SLOWER than k_nbest_forward at k = 1 beyond the spread'}")
    return met


LEGS = {"calls": (leg_calls, 400), "trace": (leg_trace, 400)}


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, None, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
