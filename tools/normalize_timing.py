#!/usr/bin/env python
"""What the normaliser costs beside the tokenizer it feeds (python tools/normalize_timing.py [cfg2|cfg5] [n] [rounds]): on device-resident input,
interleaved in one process, (a) kgpu_normalize_device alone on clean text, (b) the same with 10 % of the characters half-width or full-width,
(c) kgpu_tokenize_device alone on the clean batch.  Prints GB/s of input for (a) and (b), and (a) / (c); medians and minima over the rounds.
One context, one batch in flight: the latency of the three launches, not what several contexts overlap to.

One leg run by tools/measure.py, a process of its own under a time limit; the rounds are measure.alternated() with a device synchronize ahead of each call."""
import measure


def leg(say, kind, n, rounds):
    import numpy as np
    import torch

    from kanpyo_amd import normalize_host, synth
    from kanpyo_amd.device import DeviceContext

    n = n or (16384 if kind == "cfg2" else 256)
    sd, tok, _, _ = measure.synthetic_tokenizer()
    clean = [normalize_host(x).decode() for x in synth.make_corpus(sd, n, 1, kind)]   # (the synthetic corpus holds a few code points NFKC changes: clean means none)
    rng = np.random.default_rng(5)
    mixed = [measure.dirty(s, rng) for s in clean]
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    c, m = measure.Resident(ctx, clean), measure.Resident(ctx, mixed)
    ncap = 3 * max(c.total, m.total) + 64
    d_text, d_toff, d_st = torch.empty(ncap + 16, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)

    def norm(b):
        ctx.normalize(b.text.data_ptr(), b.offsets.data_ptr(), n, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), "NFKC")
        return ctx.sync_normalize()

    arms = {"a": lambda: norm(c), "b": lambda: norm(m), "c": c.tokenize}
    for f in arms.values():   # warm-up: tables uploaded, scratch sized, clocks up
        for _ in range(3):
            f()
    assert norm(c) == c.total, "clean text must come out as it went in"
    times = measure.alternated(arms, rounds, before=torch.cuda.synchronize)
    med, low = {k: measure.summary(v)[0] for k, v in times.items()}, {k: min(v) for k, v in times.items()}
    say(f"{kind}: {n} sentences, {c.total} clean bytes, {m.total} bytes with 10 % half-/full-width; {rounds} interleaved rounds, one batch in flight")
    say(f"  (a) normalise clean: median {med['a'] * 1e6:.0f} us (min {low['a'] * 1e6:.0f}) = {c.total / med['a'] / 1e9:.2f} GB/s")
    say(f"  (b) normalise mixed: median {med['b'] * 1e6:.0f} us (min {low['b'] * 1e6:.0f}) = {m.total / med['b'] / 1e9:.2f} GB/s")
    say(f"  (c) tokenize clean:  median {med['c'] * 1e6:.0f} us (min {low['c'] * 1e6:.0f})")
    say(f"  (a) / (c) = {med['a'] / med['c']:.3f}   (b) / (c) = {med['b'] / med['c']:.3f}")
    return True


if __name__ == "__main__":
    ap = measure.parser(__doc__)
    ap.add_argument("kind", nargs="?", default="cfg2")
    ap.add_argument("n", nargs="?", type=int, default=0)
    ap.add_argument("rounds", nargs="?", type=int, default=15)
    args = ap.parse_args()
    measure.main(__file__, args, {"measure": (lambda say: leg(say, args.kind, args.n, args.rounds), 400)}, leg_args=[args.kind, str(args.n), str(args.rounds)])
