#!/usr/bin/env python
"""What the edit records cost beside the plain normaliser, and what the span kernel costs (python tools/align_timing.py [cfg2|cfg5] [n] [rounds] [reps]):
on device-resident input, interleaved in one process, one context with one batch in flight -- the method of tools/normalize_timing.py --
  (a) kgpu_normalize_device on clean text        (A) kgpu_normalize_device_aligned on the same
  (b) ... with 10 % of the characters half-width or full-width        (B) the aligned call on the same
  (s) kgpu_source_spans_device over the records of a 4096-sentence batch of the mixed text (normalised with its edits and tokenized once, outside the timing)
Every repetition is `rounds` interleaved rounds; its medians are printed, and at the end the spread of the medians over the repetitions.

One leg run by tools/measure.py, a process of its own under a time limit; the repetitions are measure.interleaved() with a device synchronize ahead of each call."""
import measure


def leg(say, kind, n, rounds, reps):
    import numpy as np
    import torch

    from kanpyo_amd import normalize_host, synth
    from kanpyo_amd.device import DeviceContext

    n = n or (16384 if kind == "cfg2" else 256)
    sd, tok, _, _ = measure.synthetic_tokenizer()
    clean = [normalize_host(x).decode() for x in synth.make_corpus(sd, n, 1, kind)]
    rng = np.random.default_rng(5)
    mixed = [measure.dirty(s, rng) for s in clean]
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    c, m = measure.Resident(ctx, clean), measure.Resident(ctx, mixed)
    ncap, ecap = 3 * max(c.total, m.total) + 64, max(c.total, m.total)
    d_text, d_toff, d_st = torch.empty(ncap + 16, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    d_edits, d_eoff = torch.empty(ecap * 24 + 24, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)

    def norm(b):
        ctx.normalize(b.text.data_ptr(), b.offsets.data_ptr(), n, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), "NFKC")
        return ctx.sync_normalize()

    def aligned(b, k=n):
        ctx.normalize_aligned(b.text.data_ptr(), b.offsets.data_ptr(), k, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), d_edits.data_ptr(), ecap, d_eoff.data_ptr(), "NFKC")
        return ctx.sync_normalize_aligned()

    # the span kernel's batch: the first 4096 sentences (all of them when the batch has fewer) of the mixed text, normalised with edits and tokenized
    ns = min(n, 4096)
    nbytes, nedits = aligned(m, ns)
    tcap = nbytes + ns + 64
    d_tok, d_koff, d_kst = torch.empty((tcap, 6), dtype=torch.int32, device=dev), torch.empty(ns + 1, dtype=torch.int64, device=dev), torch.empty(ns, dtype=torch.uint8, device=dev)
    s_text, s_toff, s_edits, s_eoff = d_text.clone(), d_toff[: ns + 1].clone(), d_edits.clone(), d_eoff[: ns + 1].clone()
    ctx.tokenize(s_text.data_ptr(), s_toff.data_ptr(), ns, nbytes, d_tok.data_ptr(), tcap, d_koff.data_ptr(), d_kst.data_ptr())
    ntok = ctx.sync()
    d_spans = torch.empty((tcap, 4), dtype=torch.int32, device=dev)

    def spans():
        ctx.source_spans(d_tok.data_ptr(), d_koff.data_ptr(), ns, s_edits.data_ptr(), s_eoff.data_ptr(), d_spans.data_ptr(), tcap)
        return ctx.sync_lines()

    arms = {"a": lambda: norm(c), "A": lambda: aligned(c), "b": lambda: norm(m), "B": lambda: aligned(m), "s": spans}
    for f in arms.values():   # warm-up: tables uploaded, scratch sized, clocks up
        for _ in range(3):
            f()
    assert norm(c) == c.total and aligned(c) == (c.total, 0), "clean text must come out as it went in, without edits"
    say(f"{kind}: {n} sentences, {c.total} clean bytes, {m.total} bytes with 10 % half-/full-width ({aligned(m)[1]} edits); spans: {ns} sentences, {ntok} records, {nedits} edits")
    say(f"{reps} repetitions of {rounds} interleaved rounds, one batch in flight; medians in us")
    meds = {k: [x * 1e6 for x in v] for k, v in measure.interleaved(arms, reps, rounds, before=torch.cuda.synchronize).items()}
    for r in range(reps):
        say(f"  rep {r}: " + "  ".join(f"({k}) {meds[k][r]:.1f}" for k in arms) + f"   A/a {meds['A'][r] / meds['a'][r]:.3f}  B/b {meds['B'][r] / meds['b'][r]:.3f}")
    for k in arms:
        v = meds[k]
        say(f"  ({k}) median of medians {measure.summary(v)[0]:.1f} us, min {min(v):.1f}, max {max(v):.1f}, spread {measure.summary(v)[1] * 100:.1f} %")
    ra, rb = ([x / y for x, y in zip(meds[p], meds[q])] for p, q in (("A", "a"), ("B", "b")))
    say(f"  A/a: median {measure.summary(ra)[0]:.3f} (min {min(ra):.3f}, max {max(ra):.3f})   B/b: median {measure.summary(rb)[0]:.3f} (min {min(rb):.3f}, max {max(rb):.3f})")
    say(f"  spans: {measure.summary(meds['s'])[0]:.1f} us for {ntok} records of {ns} sentences")
    return True


if __name__ == "__main__":
    ap = measure.parser(__doc__)
    ap.add_argument("kind", nargs="?", default="cfg2")
    ap.add_argument("n", nargs="?", type=int, default=0)
    ap.add_argument("rounds", nargs="?", type=int, default=15)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    measure.main(__file__, args, {"measure": (lambda say: leg(say, args.kind, args.n, args.rounds, args.reps), 500)},
                 leg_args=[args.kind, str(args.n), str(args.rounds), str(args.reps)])
