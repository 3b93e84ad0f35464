#!/usr/bin/env python
"""The wakati output's rates (kgpu_words.hip and the words entry points) beside the `kanpyo tokenize` lines on cfg 2: 100k sentences, batches of
4096, 8 contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.

    python tools/words_rate.py [--out profiles/experiments/words_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; a requirement not met lets the run go on, trouble ends it):
  host     kgpu_tokenize_batch_words against kgpu_tokenize_batch_lines through measure.alternated(): medians, sentences/s and GB/s of text.
           Required: the words median is not below the lines median of the same run.  Then the DROP [助詞, 助動詞, 記号] and the field 7 handles,
           for what the table lookup and the compaction cost (no threshold).
  device   records alone, records + lines render, records + words render through measure.pipeline_rates() (measure.pipelined() with the render as the
           consumer).  Required: the words ratio (to records alone) is above the lines ratio of the same run.
  trace    measure.trace() over a child that runs the device leg once per render: microseconds per 4096-sentence batch of k_words_* beside
           k_lines_*, and the bytes moved per token (no threshold)."""
import numpy as np

import measure

N, BATCH, Q = 100_000, 4096, 8
POS_DROP = ("助詞", "助動詞", "記号")


def setup():
    from kanpyo_amd import synth

    sd, tok, _, _ = measure.synthetic_tokenizer()
    return tok, synth.make_corpus(sd, N, 1, "cfg2")


def lines_render(c, args, out, out_off):
    c.format_lines(*args, out.data_ptr(), out.numel(), out_off.data_ptr())


def words_render(w):
    return lambda c, args, out, out_off: c.format_words(w, *args, out.data_ptr(), out.numel(), out_off.data_ptr())


def leg_device(say):
    tok, sents = setup()
    out, counts = measure.pipeline_rates(tok, sents, BATCH, Q, {"records": None, "lines": lines_render, "words": words_render(tok.words())}, reps=3)
    med = {k: measure.summary(v)[0] for k, v in out.items()}
    for k in ("records", "lines", "words"):
        say(f"device-resident, {'records alone' if k == 'records' else 'records + ' + k + ' render':<24}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    rl, rw = med["lines"] / med["records"], med["words"] / med["records"]
    tokens, text = counts["words"]
    say(f"  lines ratio {rl:.2f}, words ratio {rw:.2f} of records alone; required: words above lines: {'met' if rw > rl else 'NOT MET'}")
    say(f"  words: {tokens} tokens, {text} bytes of text: {text / N:.0f} bytes per sentence, {text / tokens:.2f} bytes per token (lines: {counts['lines'][1] / counts['lines'][0]:.1f})")
    return rw > rl


def trace_child():
    tok, sents = setup()
    _, counts = measure.pipeline_rates(tok, sents, BATCH, Q, {"lines": lines_render, "words": words_render(tok.words())}, reps=1)
    print(f"COUNTS {counts['words'][0]} {counts['lines'][1]} {counts['words'][1]} {sum(len(s.encode()) for s in sents)}", flush=True)


def leg_trace(say):
    stdout, ks = measure.trace(__file__, ["--leg", "trace-child"], 400)
    tokens, text_lines, text_words, in_bytes = (int(x) for x in [ln for ln in stdout.splitlines() if ln.startswith("COUNTS ")][-1].split()[1:])
    # the scan is shared: its calls are both renders', half each (warm-up + one run per render)
    for k in sorted(ks):
        if k.startswith("k_lines_") or k.startswith("k_words_"):
            c, ns = ks[k]
            say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = measure.per_call(ks, "k_lines_scan")
    per = {p: sum(measure.per_call(ks, f"k_{p}_{s}") for s in ("len", "write")) + scan for p in ("lines", "words")}
    say(f"  kernel time per 4096-sentence batch (len + scan + write): lines {per['lines'] / 1e3:.1f} us, words {per['words'] / 1e3:.1f} us")
    # bytes moved: the 24-byte records read by both passes, per token the offsets pair (lines) or the 8-byte row entry (words) in both passes, the source
    # bytes (surfaces from the input; the lines' features = their text less surfaces, "EOS", tab and newline), the text written, 32 bytes of offsets a sentence
    feat = text_lines - tokens * 2 - in_bytes - 3 * N   # (tokens counts the EOS records, whose surface is the literal)
    moved = {"lines": tokens * (24 + 8) * 2 + in_bytes + feat + text_lines + N * 32, "words": tokens * 24 * 2 + (tokens - N) * 8 * 2 + in_bytes + text_words + N * 32}
    nb = len(range(0, N, BATCH))
    for p in ("lines", "words"):
        say(f"  {p} (a model from the counts above, not hardware counters): {moved[p] / 1e6:.0f} MB moved for {N} sentences = {moved[p] / tokens:.0f} B per token ({(text_lines if p == 'lines' else text_words) / tokens:.1f} of them text written) "
            f"-> {moved[p] / (per[p] * nb):.0f} GB/s of kernel time")
    return True


def leg_host(say):
    from kanpyo_amd.tokenizer import pack_sentences

    tok, sents = setup()
    utf8, offs = pack_sentences(sents)
    handles = {"words": tok.words(), "words, DROP 助詞 助動詞 記号": tok.words(drop=POS_DROP), "words, field 7": tok.words(field=7)}
    calls = {"lines": tok.tokenize_lines_packed}
    calls.update({k: h.render_packed for k, h in handles.items()})
    outs, sizes = {}, {}
    for k, f in calls.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = f(utf8, offs)
        sizes[k] = first.size
        outs[k] = (np.empty(first.size, dtype=np.uint8), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
        f(utf8, offs, out=outs[k])
    ts = measure.alternated({k: (lambda k=k, f=f: f(utf8, offs, out=outs[k])) for k, f in calls.items()})
    med = {k: measure.summary(v)[0] for k, v in ts.items()}
    say(f"host in / text out, {N} sentences, {int(offs[-1])} input bytes, five windows each, alternated:")
    for k in calls:
        say(f"  {k:<30} {N / med[k] / 1e6:6.2f} M sentences/s, {sizes[k] / med[k] / 1e9:5.2f} GB/s of text, {sizes[k]} bytes = {sizes[k] / int(offs[-1]):.2f} per input byte"
            f"  (windows: {', '.join(f'{N / x / 1e6:.1f}' for x in ts[k])})")
    ok = med["words"] <= med["lines"]
    say(f"  required: the words median is not below the lines median: {N / med['words'] / 1e6:.2f} vs {N / med['lines'] / 1e6:.2f} M sentences/s = "
        f"{med['lines'] / med['words']:.2f} x: {'met' if ok else 'NOT MET'}")
    return ok


LEGS = {"host": (leg_host, 500), "device": (leg_device, 400), "trace": (leg_trace, 500)}


def header():
    return (f"# tools/words_rate.py: cfg 2, {N} sentences, batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
            f"no filter unless named; library {measure.library_hash()}")


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, header, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
