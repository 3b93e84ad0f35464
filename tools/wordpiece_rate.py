#!/usr/bin/env python
"""The WordPiece ids' rates (kgpu_wordpiece.hip behind the encode entry points) beside the plain encode on cfg 2: 100k sentences, batches of 4096, 8
contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.  The layout is tools/encode_rate.py's.

    python tools/wordpiece_rate.py [--out profiles/experiments/wordpiece_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; a criterion not met lets the run go on, trouble ends it):
  host     THE YARDSTICK: a list in which every corpus word is whole (the whole read-out of a count of the corpus).  kgpu_encode_batch on a
           WordPiece handle of that list against the plain handle's -- whose kernels are the plain encode's, untouched -- through
           measure.alternated(): medians and spreads.  Criterion: the WordPiece median lies within the plain call's own spread of the plain
           median.  The ids of the two calls are compared as well.
  device   a BERT-like list of 32k entries (specials, the top words, then the corpus's characters c and ##c): the share of multi-piece and [UNK]
           tokens and the ids per token (by Vocab.split_words over the count's read-out, weighted by the counts), and records alone, records +
           plain ragged encode, + WordPiece ragged, + WordPiece padded at width 64 through measure.pipeline_rates(), medians of three; the ratios to
           records alone.
  trace    measure.trace() over a child that runs the device leg once per consumer: microseconds per 4096-sentence batch of k_wordpiece_*
           beside k_encode_* (no threshold)."""
import numpy as np

import measure

N, BATCH, Q, WIDTH = 100_000, 4096, 8, 64
LIST_SIZE = 32000
SPECIALS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"]


def setup():
    """-> tok, sents, words handle, the corpus's (word, count) read-out, the packed corpus."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, N, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    utf8, offs = pack_sentences(sents)
    k.add_packed(utf8, offs)
    counts = k.most_common()
    k.close()
    return tok, sents, w, counts, (utf8, offs)


def characters(word):
    starts = [i for i in range(len(word)) if i == 0 or word[i] & 0xC0 != 0x80] + [len(word)]
    return [word[a:b] for a, b in zip(starts, starts[1:])]


def bert_like(counts):
    """Specials, then the characters of the corpus as c and ##c, and the most frequent words in front of them up to LIST_SIZE entries."""
    chars = sorted({c for word, _ in counts for c in characters(word)})
    room = max(LIST_SIZE - len(SPECIALS) - 2 * len(chars), 0)
    head = [word for word, _ in counts if word not in SPECIALS][:room]
    seen = set(SPECIALS) | set(head)
    return SPECIALS + head + [c for c in chars if c not in seen] + [b"##" + c for c in chars if b"##" + c not in seen]


def leg_host(say):
    from kanpyo_amd.vocab import Vocab

    tok, sents, w, counts, (utf8, offs) = setup()
    words = SPECIALS + [word for word, _ in counts if word not in SPECIALS]
    handles = {"plain": Vocab(w, words, 1), "wordpiece": Vocab(w, words, 1, wordpiece=True)}
    n = N
    outs = {}
    for k, v in handles.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = v.encode_packed(utf8, offs)
        outs[k] = (np.empty(first.size, dtype=first.dtype), np.empty(n + 1, dtype=np.uint64), np.empty(n, dtype=np.uint8))
        v.encode_packed(utf8, offs, out=outs[k])
    equal = all(np.array_equal(a, b) for a, b in zip(outs["plain"], outs["wordpiece"]))
    ts = measure.alternated({k: (lambda k=k, v=v: v.encode_packed(utf8, offs, out=outs[k])) for k, v in handles.items()})
    med, spread = ({k: measure.summary(x)[i] for k, x in ts.items()} for i in (0, 1))
    say(f"host in / host out, {n} sentences, {int(offs[-1])} input bytes, five windows each, alternated; a list of {len(words)} words in which every corpus word is whole: "
        f"{handles['wordpiece'].info()} {handles['wordpiece'].wordpiece_info()}; ids equal: {equal}")
    for k in handles:
        say(f"  {k:<10} {n / med[k] / 1e6:6.2f} M sentences/s, spread {100 * spread[k]:.1f} %, {outs[k][0].size} ids  (windows: {', '.join(f'{n / x / 1e6:.1f}' for x in ts[k])})")
    ratio = med["wordpiece"] / med["plain"]
    ok = abs(ratio - 1) <= spread["plain"] and equal
    say(f"  criterion: the WordPiece median within the plain call's own spread of the plain median: WordPiece takes {ratio:.3f} x the plain call's time, "
        f"allowed 1 +- {spread['plain']:.3f}: {'met' if ok else 'NOT MET'}")
    return ok


def device_handles(w, counts):
    from kanpyo_amd.vocab import Vocab

    words = bert_like(counts)
    return words, Vocab(w, words, 1), Vocab(w, words, 1, wordpiece=True)


def encode(v, width=0):
    return lambda c, args, out, out_off: c.encode(v, *args, out.data_ptr(), out.numel() // 4, out_off.data_ptr(), width=width, pad_id=0)


LABEL = {"records": "records alone", "plain": "records + plain ragged encode", "ragged": "records + WordPiece ragged", "padded": f"records + WordPiece padded, width {WIDTH}"}


def leg_device(say):
    tok, sents, w, counts, _ = setup()
    words, plain, wp = device_handles(w, counts)
    # the shares, by the library's host split over the distinct words, weighted by their counts
    listed = set(words)
    splits = wp.split_words([word for word, _ in counts])
    tokens = sum(c for _, c in counts)
    multi = sum(c for (word, c), s in zip(counts, splits) if len(s) > 1)
    unks = sum(c for (word, c), s in zip(counts, splits) if len(s) == 1 and word not in listed)
    ids = sum(c * len(s) for (_, c), s in zip(counts, splits))
    say(f"BERT-like list of {len(words)} entries: {wp.info()} {wp.wordpiece_info()}")
    say(f"  {tokens} kept tokens: {100 * multi / tokens:.2f} % multi-piece, {100 * unks / tokens:.2f} % [UNK], {ids / tokens:.3f} ids per token")
    out, got = measure.pipeline_rates(tok, sents, BATCH, Q, {"records": None, "plain": encode(plain), "ragged": encode(wp), "padded": encode(wp, WIDTH)}, reps=3)
    med = {k: measure.summary(x)[0] for k, x in out.items()}
    for k in out:
        say(f"device-resident, {LABEL[k]:<40}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    say("  ratios to records alone: " + ", ".join(f"{k} {med[k] / med['records']:.2f}" for k in ("plain", "ragged", "padded")))
    say(f"  {got['ragged'][0]} tokens; plain: {got['plain'][1]} ids; WordPiece ragged: {got['ragged'][1]} ids")
    return True


def trace_child():
    tok, sents, w, counts, _ = setup()
    _, plain, wp = device_handles(w, counts)
    measure.pipeline_rates(tok, sents, BATCH, Q, {"plain": encode(plain), "ragged": encode(wp), "padded": encode(wp, WIDTH)}, reps=1)


def leg_trace(say):
    _, ks = measure.trace(__file__, ["--leg", "trace-child"], 400)
    for k in sorted(ks):
        if k.startswith(("k_lines_scan", "k_wordpiece_", "k_encode_")):
            c, ns = ks[k]
            say(f"  {k:<18} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = measure.per_call(ks, "k_lines_scan")   # (shared by the consumers)
    per = {p: sum(measure.per_call(ks, f"k_{p}_{s}") for s in ("len", "write")) + scan for p in ("encode", "wordpiece")}
    say(f"  kernel time per 4096-sentence batch (len + scan + write): plain encode {per['encode'] / 1e3:.1f} us, WordPiece {per['wordpiece'] / 1e3:.1f} us "
        f"(k_wordpiece_write's figure averages the ragged and the padded runs)")
    return True


LEGS = {"host": (leg_host, 500), "device": (leg_device, 500), "trace": (leg_trace, 500)}


def header():
    return (f"# tools/wordpiece_rate.py: cfg 2, {N} sentences, batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
            f"no filter; library {measure.library_hash()}")


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, header, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
