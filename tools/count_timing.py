#!/usr/bin/env python
"""What the word counts cost (kgpu_count.hip, kgpu_count_host.cpp), beside the wakati render on the same records and the wakati text call on the
same block: the synthetic 392k dictionary with synth.feature_tables, cfg 2.

    python tools/count_timing.py [--out profiles/experiments/count_words.txt] [--only kernel|host]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  kernel  measure.trace() per dispatch over a child that tokenizes ONE 4096-sentence cfg 2 batch and the 4096-sentence hot-key batch (one dictionary word
          repeated 32 times per sentence: tests/test_gpu_count.py::test_hot_key) on a context, leaves the records in HBM and then runs, REPS times each
          and in this order: the count for the surface and for the reading (field 7) on the cfg 2 records, the surface count on the hot-key records,
          and the two wakati renders (surface, field 7) on the cfg 2 records.  Kernel times are the trace's, per dispatch, medians over the
          repetitions behind the first two; the very first count of a handle (every unknown surface is new: probe, arena, claim) is quoted apart.
          The hot-key count is held against tokens / 88 per microsecond, what one global atomic per token on one address would cost at least.
  host    kgpu_count_text against kgpu_tokenize_text_words on one block of 64 MiB or more (the 100k-sentence cfg 2 corpus, repeated) through
          measure.alternated(): medians and the spread of each."""
import time

import numpy as np

import measure

BATCH, REPS, SKIP = 4096, 22, 2
ATOMICS_PER_US = 88   # one address, chip-wide (kgpu_device.h above WorkIO)


def kernel_child():
    import torch

    from kanpyo_amd import synth
    from kanpyo_amd.device import DeviceContext

    sd, tok, _, _ = measure.synthetic_tokenizer()
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    hot = synth.record_surfaces(sd)[196000]
    cfg2 = measure.Resident(ctx, synth.make_corpus(sd, BATCH, 1, "cfg2"))
    hotb = measure.Resident(ctx, [hot * 32] * BATCH)
    w_s, w_r = tok.words(), tok.words(field=7)
    text = torch.empty(8 << 20, dtype=torch.uint8, device=dev)
    text_off = torch.empty(BATCH + 1, dtype=torch.int64, device=dev)
    counted = {}
    for name, w, b in (("count surface cfg2", w_s, cfg2), ("count reading cfg2", w_r, cfg2), ("count surface hot", w_s, hotb)):
        k = w.counter()
        for _ in range(REPS):
            ctx.count_words(k, *b.args())
            counted[name] = ctx.sync_count()
        info = k.info()
        print(f"INFO {name}: {counted[name]} tokens counted per launch, {info['table_slots_used']} slots and {info['key_bytes_used']} key bytes used, "
              f"{len(k.most_common())} distinct words", flush=True)
        k.close()
    for w in (w_s, w_r):
        for _ in range(REPS):
            ctx.format_words(w, *cfg2.args(), text.data_ptr(), text.numel(), text_off.data_ptr())
            ctx.sync_lines()
    print(f"SIZES {cfg2.count} {cfg2.total} {hotb.count} {hotb.total}", flush=True)
    ctx.close()


def leg_kernel(say):
    stdout, per = measure.trace(__file__, ["--leg", "kernel-child"], 420, stats=False)
    for ln in stdout.splitlines():
        if ln.startswith("INFO "):
            say("  " + ln[5:])
    tok2, bytes2, tokh, bytesh = (int(x) for x in [ln for ln in stdout.splitlines() if ln.startswith("SIZES ")][-1].split()[1:])

    def phases(name, k):   # the dispatches of a kernel, in time order, cut into k phases of REPS
        d = per.get(name, [])
        if len(d) != k * REPS:
            raise RuntimeError(f"{name}: {len(d)} dispatches in the trace, expected {k * REPS}; kernels seen: {sorted(per)}")
        return [d[i * REPS : (i + 1) * REPS] for i in range(k)]

    med = lambda v: measure.summary(v[SKIP:])[0] / 1e3   # noqa: E731
    cw, cp = phases("k_count_words", 3), phases("k_count_publish", 3)
    wl, ww, sc = phases("k_words_len", 2), phases("k_words_write", 2), phases("k_lines_scan", 2)
    say(f"  the cfg 2 batch: {BATCH} sentences, {bytes2} bytes, {tok2} records; the hot-key batch: {BATCH} sentences, {bytesh} bytes, {tokh} records")
    count_us = {}
    for i, name in enumerate(("surface, cfg 2", "reading, cfg 2", "surface, hot key")):
        count_us[name] = med(cw[i]) + med(cp[i])
        say(f"  count {name:<17}: k_count_words {med(cw[i]):7.1f} us (min {min(cw[i][SKIP:]) / 1e3:.1f}, max {max(cw[i][SKIP:]) / 1e3:.1f}; the handle's first launch {cw[i][0] / 1e3:.1f}) "
            f"+ k_count_publish {med(cp[i]):.1f} us = {count_us[name]:.1f} us")
    words_us = {}
    for i, name in enumerate(("surface", "reading")):
        words_us[name] = med(wl[i]) + med(sc[i]) + med(ww[i])
        say(f"  wakati render {name:<8}: k_words_len {med(wl[i]):.1f} + k_lines_scan {med(sc[i]):.1f} + k_words_write {med(ww[i]):.1f} = {words_us[name]:.1f} us")
    say(f"  count / render on the same records: surface {count_us['surface, cfg 2'] / words_us['surface']:.2f}, reading {count_us['reading, cfg 2'] / words_us['reading']:.2f}")
    bound = (tokh - BATCH) / ATOMICS_PER_US
    hot_us = count_us["surface, hot key"]
    say(f"  hot key: {tokh - BATCH} counted tokens at one global atomic each on one address would take {bound:.0f} us at least ({ATOMICS_PER_US} per us); "
        f"the count takes {hot_us:.1f} us = {hot_us / bound:.3f} of that: {'well under the bound' if hot_us < bound / 4 else 'NOT well under the bound'}")
    return hot_us < bound / 4


def leg_host(say):
    from kanpyo_amd import synth

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, 100_000, 1, "cfg2")
    one = "".join(s + "\n" for s in sents).encode()
    block = np.frombuffer(one * (-(-(64 << 20) // len(one))), dtype=np.uint8)
    lines = int(np.count_nonzero(block == 10))
    w = tok.words()
    k = w.counter()
    wakati = lambda: w.render_text(block)   # noqa: E731
    count = lambda: k.add_text(block)       # noqa: E731
    text, _, _ = wakati()
    count()
    ts = measure.alternated({"wakati": wakati, "count": count})
    med, spread = ({n: measure.summary(v)[i] for n, v in ts.items()} for i in (0, 1))
    info = k.info()
    say(f"host block in, {block.size} bytes = {block.size / (1 << 20):.1f} MiB, {lines} lines; five windows each, alternated (the Python wrappers' own buffers included):")
    say(f"  kgpu_tokenize_text_words : {lines / med['wakati'] / 1e6:6.2f} M sentences/s, {med['wakati'] * 1e3:7.1f} ms median, spread {spread['wakati'] * 100:.0f} % of it "
        f"({', '.join(f'{x * 1e3:.0f}' for x in ts['wakati'])} ms); {text.size} bytes of text back")
    say(f"  kgpu_count_text          : {lines / med['count'] / 1e6:6.2f} M sentences/s, {med['count'] * 1e3:7.1f} ms median, spread {spread['count'] * 100:.0f} % of it "
        f"({', '.join(f'{x * 1e3:.0f}' for x in ts['count'])} ms); {lines} status bytes back")
    say(f"  count / wakati time: {med['count'] / med['wakati']:.2f}; the handle: {info['tokens_counted']} tokens counted in {info['sentences']} sentences, "
        f"{info['table_slots_used']} slots used, {info['overflow_tokens']} overflow tokens")
    t0 = time.perf_counter()
    n = len(k.most_common())
    say(f"  read-out of {n} distinct words (default table: 64 MiB of slots back to the host, resolved, merged, sorted): {(time.perf_counter() - t0) * 1e3:.0f} ms")
    return True


LEGS = {"kernel": (leg_kernel, 480), "host": (leg_host, 420)}


def header():
    return (f"# tools/count_timing.py: cfg 2, batches of {BATCH}, synthetic 392k dictionary + synth.feature_tables, no filter; medians of {REPS - SKIP} repetitions; "
            f"library {measure.library_hash()}")


if __name__ == "__main__":
    ap = measure.parser(__doc__)
    ap.add_argument("--only", default=None, choices=list(LEGS))
    args = ap.parse_args()
    measure.main(__file__, args, LEGS, header, {"kernel-child": kernel_child}, skip=[n for n in LEGS if args.only and n != args.only], headings=True)
