#!/usr/bin/env python
"""The vocabulary ids' rates (kgpu_encode.hip and the encode entry points) beside the wakati render on cfg 2: 100k sentences, batches of 4096, 8
contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter; the vocabulary is the whole read-out of a count of the
same corpus behind <pad> and <unk>.

    python tools/encode_rate.py [--out profiles/experiments/encode_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; a criterion not met lets the run go on, trouble ends it):
  host     kgpu_encode_batch against kgpu_tokenize_batch_words through measure.alternated(): medians and spreads.  The yardstick is the words call,
           which writes about 4.5 bytes per token where encode writes 4.  Criterion: encode is not slower than words by more than the spread of
           the words call's own five windows in this run.
  device   records alone, records + words render, records + ragged encode, records + padded encode at width 64 through measure.pipeline_rates()
           (measure.pipelined() with the consumer as a parameter), medians of three; the ratios to records alone (no threshold).
  trace    measure.trace() over a child that runs the device leg once per consumer: microseconds per 4096-sentence batch of k_encode_* beside
           k_words_* (no threshold)."""
import numpy as np

import measure

N, BATCH, Q, WIDTH = 100_000, 4096, 8, 64


def setup():
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, N, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    utf8, offs = pack_sentences(sents)
    k.add_packed(utf8, offs)
    v = k.vocabulary()
    k.close()
    return tok, sents, w, v, (utf8, offs)


def consumers_of(w, v):
    """What reads the records of a batch: nothing, the words render, the ragged and the padded encode."""
    def encode(width):
        return lambda c, args, out, out_off: c.encode(v, *args, out.data_ptr(), out.numel() // 4, out_off.data_ptr(), width=width, pad_id=0)

    return {"records": None, "words": lambda c, args, out, out_off: c.format_words(w, *args, out.data_ptr(), out.numel(), out_off.data_ptr()),
            "ragged": encode(0), "padded": encode(WIDTH)}


LABEL = {"records": "records alone", "words": "records + words render", "ragged": "records + ragged encode", "padded": f"records + padded encode, width {WIDTH}"}


def leg_device(say):
    tok, sents, w, v, _ = setup()
    out, counts = measure.pipeline_rates(tok, sents, BATCH, Q, consumers_of(w, v), reps=3)
    med = {k: measure.summary(x)[0] for k, x in out.items()}
    for k in out:
        say(f"device-resident, {LABEL[k]:<36}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    say("  ratios to records alone: " + ", ".join(f"{k} {med[k] / med['records']:.2f}" for k in ("words", "ragged", "padded")))
    say(f"  {counts['ragged'][0]} tokens; words: {counts['words'][1]} bytes of text; ragged: {counts['ragged'][1]} ids = {4 * counts['ragged'][1]} bytes; "
        f"padded: {N} x {WIDTH} ids = {4 * N * WIDTH} bytes; vocabulary: {v.info()}")
    return True


def trace_child():
    tok, sents, w, v, _ = setup()
    cons = consumers_of(w, v)
    del cons["records"]
    measure.pipeline_rates(tok, sents, BATCH, Q, cons, reps=1)


def leg_trace(say):
    _, ks = measure.trace(__file__, ["--leg", "trace-child"], 400)
    for k in sorted(ks):
        if k.startswith(("k_lines_scan", "k_words_", "k_encode_")):
            c, ns = ks[k]
            say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = measure.per_call(ks, "k_lines_scan")   # (shared by the three consumers)
    per = {p: sum(measure.per_call(ks, f"k_{p}_{s}") for s in ("len", "write")) + scan for p in ("words", "encode")}
    say(f"  kernel time per 4096-sentence batch (len + scan + write): words {per['words'] / 1e3:.1f} us, encode {per['encode'] / 1e3:.1f} us "
        f"(k_encode_write's figure averages the ragged and the padded runs)")
    return True


def leg_host(say):
    tok, sents, w, v, (utf8, offs) = setup()
    calls = {"words": w.render_packed, "encode": v.encode_packed}
    outs, sizes = {}, {}
    for k, f in calls.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = f(utf8, offs)
        sizes[k] = first.size
        outs[k] = (np.empty(first.size, dtype=first.dtype), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
        f(utf8, offs, out=outs[k])
    ts = measure.alternated({k: (lambda k=k, f=f: f(utf8, offs, out=outs[k])) for k, f in calls.items()})
    med, spread = ({k: measure.summary(x)[i] for k, x in ts.items()} for i in (0, 1))
    say(f"host in / host out, {N} sentences, {int(offs[-1])} input bytes, five windows each, alternated; vocabulary of {len(v.words)} words: {v.info()}")
    unit = {"words": "bytes of text", "encode": "ids"}
    for k in calls:
        say(f"  {k:<8} {N / med[k] / 1e6:6.2f} M sentences/s, spread {100 * spread[k]:.1f} %, {sizes[k]} {unit[k]} = {sizes[k] * (4 if k == 'encode' else 1)} bytes out"
            f"  (windows: {', '.join(f'{N / x / 1e6:.1f}' for x in ts[k])})")
    ratio = med["encode"] / med["words"]
    ok = ratio <= 1 + spread["words"]
    say(f"  criterion: encode not slower than words by more than the words call's own spread: encode takes {ratio:.3f} x the words call's time, "
        f"allowed {1 + spread['words']:.3f}: {'met' if ok else 'NOT MET'}")
    return ok


LEGS = {"host": (leg_host, 500), "device": (leg_device, 400), "trace": (leg_trace, 500)}


def header():
    return (f"# tools/encode_rate.py: cfg 2, {N} sentences, batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
            f"no filter; vocabulary = <pad>, <unk> and the whole read-out of a count of the same corpus; library {measure.library_hash()}")


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, header, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
