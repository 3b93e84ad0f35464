#!/usr/bin/env python
"""The model inputs' cost (kgpu_pack.hip, include/kanpyo_gpu.h "model inputs") beside the ragged encode step it follows, on the synthetic 392k dictionary
with a WordPiece list of every character and ##character of the corpus, [CLS] / [SEP] added by the vocabulary:
  cfg 2    16 384 sentences of about 40 characters, singles, max_length 64 and max_length 512 (one row each: the cost of the padding)
  cfg 5    256 documents of 2048 characters, singles, max_length 512, stride 128 (overlapping windows)
each without and with spans and token indices.

    python tools/pack_rate.py [--out profiles/experiments/pack_rate.txt] [--no-trace]

Two legs run by tools/measure.py, each a process of its own under a time limit (trouble in the first ends the run).  measure: ONE context with ONE
batch in flight, device-resident records tokenized once outside the timing, the two arms -- kgpu_encode_device[_spans] (ragged) and kgpu_pack_device on
what it wrote -- through measure.interleaved(), five repetitions of 15 rounds, around enqueue + kgpu_ctx_sync_lines; the median of the five medians in
us and the spread of the medians.  trace: measure.trace() over ONE arm pair, for the kernels' own time.
Both arms are three launches and one wait: a call of a few tens of microseconds is mostly that.  Two figures per row: the pack's time over the
encode's, and the pack's bytes -- read (the ids it copies, with spans 20 bytes more per element, and the offsets) plus written (12 bytes per slot,
32 with spans, and the row offsets and status) -- over its time, beside the 6.29 TB/s copy rate DESIGN.md uses."""
import measure

COPY_RATE = 6.29e12   # the chip's measured copy rate, bytes/s
REPS, ROUNDS = 5, 15
CASES = [("cfg 2 x 16384, max_length 64", "cfg2", 16384, 64, 0), ("cfg 2 x 16384, max_length 512", "cfg2", 16384, 512, 0),
         ("cfg 5 (2048 characters) x 256, max_length 512, stride 128", "cfg5", 256, 512, 128)]


def leg(say, only=None):
    """only = (case index, with spans): that one arm pair alone (the trace's child)."""
    import torch

    from kanpyo_amd import synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.pack import pack_opts

    sd, tok, _, _ = measure.synthetic_tokenizer()
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    for ci, (label, kind, n, ML, stride) in enumerate(CASES):
        if only is not None and only[0] != ci:
            continue
        sents = synth.make_corpus(sd, n, 1, kind)
        chars = sorted({c for s in sents for c in s})
        vocab = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"] + [c.encode() for c in chars] + [b"##" + c.encode() for c in chars]
        v = tok.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
        b = measure.Resident(ctx, sents)
        id_cap = b.total + 2 * n + 64   # (a piece is a character at least)
        d_ids = torch.empty(id_cap, dtype=torch.int32, device=dev)
        d_ioff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_spans = torch.empty((id_cap, 4), dtype=torch.int32, device=dev)
        d_tix = torch.empty(id_cap, dtype=torch.int32, device=dev)
        opts = pack_opts(ML, stride, "only_first", True, 2, 3, 0, trim_front=1, trim_back=1)
        d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_pst = torch.empty(n, dtype=torch.uint8, device=dev)
        for with_spans in (False, True):
            if only is not None and only[1] != with_spans:
                continue

            def encode():
                args = (v, b.text.data_ptr(), b.offsets.data_ptr(), n, b.records.data_ptr(), b.record_offsets.data_ptr(), d_ids.data_ptr(), id_cap, d_ioff.data_ptr())
                if with_spans:
                    ctx.encode_spans(*args, d_spans.data_ptr(), d_tix.data_ptr())
                else:
                    ctx.encode(*args)
                return ctx.sync_lines()

            n_ids = encode()
            row_cap = n + n_ids // max(1, ML - 2 - stride) + 8
            rows = [torch.empty((row_cap, ML), dtype=torch.int32, device=dev) for _ in range(4)]
            r_spans = torch.empty((row_cap, ML, 4), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)

            def pack():
                ctx.pack(opts, n, d_ids.data_ptr(), d_ioff.data_ptr(), n_ids, rows[0].data_ptr(), row_cap, d_roff.data_ptr(), d_pst.data_ptr(),
                         d_type_ids=rows[1].data_ptr(), d_mask=rows[2].data_ptr(), d_spans_in=d_spans.data_ptr() if with_spans else 0,
                         d_tix_in=d_tix.data_ptr() if with_spans else 0, d_spans=r_spans.data_ptr() if with_spans else 0, d_tix=rows[3].data_ptr() if with_spans else 0)
                return ctx.sync_lines()

            R = pack()
            copied = int(rows[2][:R].sum().item()) - 2 * R   # the slots that hold an element: the mask's ones without the two specials of a row
            moved = copied * 4 + (n + 1) * 8 + R * ML * 12 + (n + 1) * 8 + n + (copied * 20 + R * ML * 20 if with_spans else 0)
            med = measure.interleaved({"encode": encode, "pack": pack}, REPS, ROUNDS)
            m, sp = ({k: measure.summary(x)[i] for k, x in med.items()} for i in (0, 1))
            rate = moved / m["pack"]
            say(f"{label}, {'with' if with_spans else 'no'} spans: {n_ids} ids -> {R} rows; ragged encode {m['encode'] * 1e6:8.1f} us ({100 * sp['encode']:.1f} %), "
                f"pack {m['pack'] * 1e6:8.1f} us ({100 * sp['pack']:.1f} %), pack / encode {m['pack'] / m['encode']:.3f}; pack moves {moved} bytes: "
                f"{rate / 1e9:7.1f} GB/s = {100 * rate / COPY_RATE:.1f} % of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
        v.close()
    ctx.close()
    return True


def trace(say):
    """measure.trace() over a child that runs ONE arm pair (the largest case, cfg 2 at max_length 512): the kernels' own time per call, without the
    launches' and the wait's share of the host clock."""
    ci = 1
    for with_spans in (0, 1):
        _, ks = measure.trace(__file__, ["--leg", "trace-child", "--only", f"{ci}:{with_spans}"], 200)
        say(f"kernel trace, {CASES[ci][0]}, {'with' if with_spans else 'no'} spans: " + ", ".join(
            f"{k} {ns / 1e3 / c:.1f} us x {c}" for k, (c, ns) in sorted(ks.items()) if k.startswith(("k_pack_", "k_lines_scan", "k_wordpiece_"))))
    return True


LEGS = {"measure": (leg, 500), "trace": (trace, 500)}   # (two traced runs of 200 s at the most)


def header():
    return (f"# tools/pack_rate.py: one context, one batch in flight, {REPS} x {ROUNDS} rounds interleaved, host clock around enqueue + sync; synthetic 392k dictionary, "
            f"WordPiece list of every character and ##character; library {measure.library_hash()}")


if __name__ == "__main__":
    ap = measure.parser(__doc__, no_trace=True)
    ap.add_argument("--only", default=None, help=measure.argparse.SUPPRESS)
    args = ap.parse_args()
    only = None if args.only is None else (int(args.only.split(":")[0]), args.only.endswith(":1"))
    measure.main(__file__, args, LEGS, header, {"trace-child": lambda: leg(measure.say, only)}, skip=("trace",) if args.no_trace else ())
