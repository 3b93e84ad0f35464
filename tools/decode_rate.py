#!/usr/bin/env python
"""The text from ids' rate (kgpu_decode.hip) beside the wakati render (kgpu_words.hip) of the same batch in the same build: ONE batch of 4096 cfg 2
sentences, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.  The vocabulary is the whole read-out of a count of the
batch behind <pad> and <unk>: every word is listed, so decode writes the bytes the words render writes minus the newlines (checked here), and reads 4
bytes per element where the render reads a 24-byte record.

    python tools/decode_rate.py [--out profiles/experiments/decode_rate.txt] [--no-trace]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  device   the records and the ids stay in HBM; measure.windows() of ITERS enqueue + sync_lines pairs of one consumer on one context: medians, spreads
           and the ratio decode / words of the medians (no threshold: none has been measured before).
  trace    measure.trace() over a child that runs each consumer ITERS times: microseconds per batch of k_decode_* beside k_words_*."""
import measure

BATCH, ITERS, WINDOWS = 4096, 2000, 5   # (a window is a few tenths of a second)


def setup():
    """-> (context, {name: enqueue()}, facts): the batch tokenized and encoded once, both consumers' buffers in HBM."""
    import torch

    from kanpyo_amd import synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, BATCH, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    k.add_packed(*pack_sentences(sents))
    v = k.vocabulary()
    k.close()
    dev = torch.device("cuda", 0)
    c = DeviceContext(tok)
    b = measure.Resident(c, sents)
    n = b.n
    ids, ioff = torch.empty(b.cap, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    text_w, toff_w = torch.empty(16 << 20, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    text_d, toff_d, st_d = torch.empty(16 << 20, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.encode(v, *b.args(), ids.data_ptr(), b.cap, ioff.data_ptr())
    n_ids = c.sync_lines()
    calls = {
        "words": lambda: c.format_words(w, b.text.data_ptr(), b.offsets.data_ptr(), n, b.records.data_ptr(), b.record_offsets.data_ptr(), text_w.data_ptr(), text_w.numel(), toff_w.data_ptr()),
        "decode": lambda: c.decode(v, ids.data_ptr(), ioff.data_ptr(), n, text_d.data_ptr(), text_d.numel(), toff_d.data_ptr(), st_d.data_ptr()),
    }
    size = {}
    for name, f in calls.items():   # once each: the first decode uploads the handle's id -> word table
        f()
        size[name] = c.sync_lines()
    # every word is listed: the decoded lines are the rendered lines without their newlines
    a, ao = text_w[: size["words"]].cpu().numpy().tobytes(), toff_w.cpu().tolist()
    d, do = text_d[: size["decode"]].cpu().numpy().tobytes(), toff_d.cpu().tolist()
    same = all(a[ao[i] : ao[i + 1] - 1] == d[do[i] : do[i + 1]] for i in range(n)) and not bool(st_d.any())
    facts = dict(n=n, input_bytes=b.total, tokens=b.count, ids=n_ids, words_bytes=size["words"], decode_bytes=size["decode"], same=same, vocabulary=len(v.words))
    keep = (tok, w, v, b, ids, ioff, text_w, toff_w, text_d, toff_d, st_d)
    return c, calls, facts, keep


def synced(c, f):
    def call():
        f()
        c.sync_lines()

    return call


def leg_device(say):
    c, calls, facts, _keep = setup()
    say(f"one batch: {facts['n']} sentences, {facts['input_bytes']} input bytes, {facts['tokens']} records, {facts['ids']} ids, vocabulary of {facts['vocabulary']} words; "
        f"words render {facts['words_bytes']} bytes, decode {facts['decode_bytes']} bytes; decoded lines == rendered lines minus the newline: {facts['same']}")
    if not facts["same"] or facts["decode_bytes"] != facts["words_bytes"] - facts["n"]:
        raise RuntimeError("the decoded lines are not the rendered lines")
    ts = measure.windows({k: synced(c, f) for k, f in calls.items()}, ITERS, WINDOWS)
    med, spread = ({k: measure.summary(x)[i] for k, x in ts.items()} for i in (0, 1))
    for k in calls:
        say(f"  {k:<7} {med[k] * 1e6:7.1f} us per batch (enqueue + sync, {ITERS} per window), spread {100 * spread[k]:.1f} %  (windows: {', '.join(f'{x * 1e6:.1f}' for x in ts[k])})")
    say(f"  ratio decode / words of the medians: {med['decode'] / med['words']:.3f}  (the words render's own spread: {100 * spread['words']:.1f} %)")
    return True


def trace_child():
    c, calls, _, _keep = setup()
    for f in calls.values():
        for _ in range(ITERS):
            f()
            c.sync_lines()


def leg_trace(say):
    _, ks = measure.trace(__file__, ["--leg", "trace-child"], 400)
    for k in sorted(ks):
        if k.startswith(("k_lines_scan", "k_words_", "k_decode_")):
            n, ns = ks[k]
            say(f"  {k:<16} {n} calls, {ns / 1e3 / n:8.1f} us per call")
    scan = measure.per_call(ks, "k_lines_scan")   # (shared by the consumers)
    per = {p: sum(measure.per_call(ks, f"k_{p}_{s}") for s in ("len", "write")) + scan for p in ("words", "decode")}
    say(f"  kernel time per {BATCH}-sentence batch (len + scan + write): words {per['words'] / 1e3:.1f} us, decode {per['decode'] / 1e3:.1f} us, ratio {per['decode'] / per['words']:.3f}")
    return True


LEGS = {"device": (leg_device, 400), "trace": (leg_trace, 500)}


def header():
    return (f"# tools/decode_rate.py: cfg 2, one batch of {BATCH} sentences, one context; synthetic 392k dictionary + synth.feature_tables; surface field, no filter; "
            f"vocabulary = <pad>, <unk> and the whole read-out of a count of the batch; library {measure.library_hash()}")


if __name__ == "__main__":
    args = measure.parser(__doc__, no_trace=True).parse_args()
    measure.main(__file__, args, LEGS, header, {"trace-child": trace_child}, skip=("trace",) if args.no_trace else ())
