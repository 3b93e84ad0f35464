#!/usr/bin/env python
"""The user dictionary call's rate (kgpu_tokenize_batch_user, kgpu_user.hip) on the first 4096 sentences of the cfg 2 corpus (the synthetic 392k
dictionary), one chunk of 1024 after the other, in search mode, with E = 0, 1 000 and 100 000 entries drawn from the corpus's own substrings (1 to 6
characters: every one matches somewhere).  The yardsticks come from the same run: kgpu_tokenize_batch_mode in search mode -- k_mode_forward, which
kgpu_user.hip leaves as it was -- and the lattice launch, k_tokenize_general with BatchArgs::keep_lattice, which every chunk of either call pays.

    python tools/userdict_rate.py [--out profiles/experiments/userdict.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  calls    per arm the call's wall time (host memory in, host memory out; after a warm-up call, which grows the arena) -> sentences/s, with the user
           tokens among the records.
  trace    measure.trace() over a child that makes the same calls, kernel tracing alone, in a run of its own: per call the time of k_tokenize_general and
           of k_mode_forward or k_user_forward, each with its spread over the calls, and k_user_forward over k_mode_forward.  No figure is asked of it."""
import time

import measure

SIZES = (0, 1000, 100000)
ARMS = ("mode",) + tuple(f"user E = {e}" for e in SIZES)
CALLS = 5
SENTENCES = 4096
MODE = "search"


def entries_of(sents, n, rows, cols, seed=7):
    """n entries whose keys are substrings of the corpus, 1 to 6 characters, ids over the whole matrix, costs around a word's."""
    import random

    rng = random.Random(seed)
    out = []
    while len(out) < n:
        s = rng.choice(sents)
        if not s:
            continue
        a = rng.randrange(len(s))
        out.append((s[a : a + rng.randint(1, 6)], rng.randrange(cols), rng.randrange(rows), rng.randint(2000, 9000)))
    return out


def setup():
    from kanpyo_amd import UserDict, synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, SENTENCES, 1, "cfg2")
    info = tok.info()
    uds = [UserDict(tok, entries_of(sents, e, info["conn_rows"], info["conn_cols"])) for e in SIZES]
    return tok, sents, pack_sentences(sents), uds


def chunks_of(offs) -> int:
    """The chunks the call cuts this input into: at most 256 KiB and 1024 sentences each (kgpu_lattice_call.h over cut_chunk)."""
    o, n, done, chunks = offs.tolist(), len(offs) - 1, 0, 0
    while done < n:
        m = 0
        while done + m < n and m < 1024 and (m == 0 or o[done + m + 1] - o[done] <= 256 << 10):
            m += 1
        done, chunks = done + m, chunks + 1
    return chunks


def run_calls(tok, utf8, offs, uds, timed=None):
    """A warm-up call per arm, then CALLS calls per arm in the order of ARMS, each ONE call of the library -> per arm (records, user records)."""
    calls = [lambda cap=None: tok.tokenize_mode_packed(utf8, offs, MODE, token_capacity=cap)] + [lambda cap=None, u=u: tok.tokenize_user_packed(utf8, offs, u, MODE, token_capacity=cap) for u in uds]
    room = [len(c()[0]) for c in calls]
    sizes = {}
    for arm, call, cap in zip(ARMS, calls, room):
        for _ in range(CALLS):
            t0 = time.perf_counter()
            got = call(cap)
            if timed is not None:
                timed.setdefault(arm, []).append(time.perf_counter() - t0)
        sizes[arm] = (len(got[0]), int((got[0]["cls"] == 3).sum()))
    return sizes


def leg_calls(say):
    say(f"# tools/userdict_rate.py: synthetic 392k dictionary, {MODE} mode; {CALLS} calls per arm behind a warm-up call; library {measure.library_hash()}")
    tok, sents, (utf8, offs), uds = setup()
    for e, u in zip(SIZES, uds):
        say(f"  E = {e}: {u.info()}")
    timed = {}
    sizes = run_calls(tok, utf8, offs, uds, timed)
    say(f"cfg2: {len(sents)} sentences, {int(offs[-1])} bytes, {chunks_of(offs)} chunks")
    base = measure.summary(timed["mode"])[0]
    for arm in timed:
        m, spread = measure.summary(timed[arm])
        say(f"  {arm:<16} {m * 1e3:9.2f} ms per call, spread {100 * spread:.0f} %  -> {len(sents) / m:10.0f} sentences/s; {sizes[arm][0]} records, {sizes[arm][1]} of them user tokens; "
            f"call / mode call = {m / base:.2f}")
    for u in uds:
        u.close()
    tok.close()
    return True


def trace_child():
    tok, _, (utf8, offs), uds = setup()
    run_calls(tok, utf8, offs, uds)
    print(chunks_of(offs))


def leg_trace(say):
    out, ds = measure.trace(__file__, ["--leg", "trace-child"], 500, stats=False)
    chunks = int(out.split()[-1])
    per = CALLS * chunks
    need = {"k_mode_forward": per, "k_user_forward": len(SIZES) * per, "k_tokenize_general": len(ARMS) * per}
    if any(len(ds.get(name, [])) < c for name, c in need.items()):
        say(f"  fewer dispatches than {CALLS} calls of {chunks} chunks make: {[(name, len(ds.get(name, []))) for name in need]}")
        return False

    def calls_of(name, i, arms):
        """Per call the kernel's time in us: the dispatches of arm i of `arms` timed arms, counted from the end (the warm-up calls' left out)."""
        d = ds[name]
        tail = d[len(d) - (arms - i) * per : len(d) - (arms - i - 1) * per]
        return [sum(tail[c * chunks : (c + 1) * chunks]) / 1e3 for c in range(CALLS)]

    say(f"cfg2: kernel time per call of {chunks} chunks in us, median and spread over {CALLS} calls (rocprofv3 --kernel-trace, a run of its own)")
    # (the timed calls of an arm lie in front of the next arm's: the mode arm's k_mode_forward dispatches are its last `per`)
    lattice = [measure.summary(calls_of("k_tokenize_general", i, len(ARMS))) for i in range(len(ARMS))]
    mf, mf_spread = measure.summary(calls_of("k_mode_forward", 0, 1))
    say(f"  {'mode':<16} k_tokenize_general {lattice[0][0]:9.1f} ({100 * lattice[0][1]:.0f} %)   k_mode_forward {mf:9.1f} ({100 * mf_spread:.0f} %)")
    for i, e in enumerate(SIZES):
        fw, fw_spread = measure.summary(calls_of("k_user_forward", i, len(SIZES)))
        say(f"  {ARMS[1 + i]:<16} k_tokenize_general {lattice[1 + i][0]:9.1f} ({100 * lattice[1 + i][1]:.0f} %)   k_user_forward {fw:9.1f} ({100 * fw_spread:.0f} %)"
            f"   k_user_forward / k_mode_forward = {fw / mf:.2f}")
    return True


LEGS = {"calls": (leg_calls, 500), "trace": (leg_trace, 560)}


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, None, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
