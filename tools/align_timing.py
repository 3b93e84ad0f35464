#!/usr/bin/env python
"""What the edit records cost beside the plain normaliser, and what the span kernel costs (python tools/align_timing.py [cfg2|cfg5] [n] [rounds] [reps]):
on device-resident input, interleaved in one process, one context with one batch in flight -- the method of tools/normalize_timing.py --
  (a) kgpu_normalize_device on clean text        (A) kgpu_normalize_device_aligned on the same
  (b) ... with 10 % of the characters half-width or full-width        (B) the aligned call on the same
  (s) kgpu_source_spans_device over the records of a 4096-sentence batch of the mixed text (normalised with its edits and tokenized once, outside the timing)
Every repetition is `rounds` interleaved rounds; its medians are printed, and at the end the spread of the medians over the repetitions."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from kanpyo_amd import Tokenizer, normalize_host, synth
from kanpyo_amd.device import DeviceContext
from kanpyo_amd.tokenizer import pack_sentences
kind = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
n = int(sys.argv[2]) if len(sys.argv) > 2 else (16384 if kind == "cfg2" else 256)
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 15
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
HALF = "ｱｲｳｴｵｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾅﾆﾇﾈﾉ"
FULL = "ＡＢＣＤＥＦＧＨＩＪ０１２３４５６７８９"
def dirty(s, rng):   # every tenth character, on average, becomes a half-width kana or a full-width letter or digit
    pool = HALF + FULL
    return "".join(pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.1 else c for c in s)
sd = synth.build_dict(); clean = [normalize_host(x).decode() for x in synth.make_corpus(sd, n, 1, kind)]
rng = np.random.default_rng(5); mixed = [dirty(s, rng) for s in clean]
tok = Tokenizer(sd.dict); dev = torch.device("cuda", 0); ctx = DeviceContext(tok)
def resident(sents):
    utf8, offs = pack_sentences(sents)
    return torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev), int(offs[-1])
cu, co, cbytes = resident(clean); mu, mo, mbytes = resident(mixed)
ncap = 3 * max(cbytes, mbytes) + 64; ecap = max(cbytes, mbytes)
d_text = torch.empty(ncap + 16, dtype=torch.uint8, device=dev); d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev); d_st = torch.empty(n, dtype=torch.uint8, device=dev)
d_edits = torch.empty(ecap * 24 + 24, dtype=torch.uint8, device=dev); d_eoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
def norm(u, o):
    ctx.normalize(u.data_ptr(), o.data_ptr(), n, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), "NFKC"); return ctx.sync_normalize()
def aligned(u, o, m=n):
    ctx.normalize_aligned(u.data_ptr(), o.data_ptr(), m, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), d_edits.data_ptr(), ecap, d_eoff.data_ptr(), "NFKC")
    return ctx.sync_normalize_aligned()
# the span kernel's batch: the first 4096 sentences (all of them when the batch has fewer) of the mixed text, normalised with edits and tokenized
ns = min(n, 4096)
nbytes, nedits = aligned(mu, mo, ns)
tcap = nbytes + ns + 64
d_tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev); d_koff = torch.empty(ns + 1, dtype=torch.int64, device=dev); d_kst = torch.empty(ns, dtype=torch.uint8, device=dev)
s_text, s_toff, s_edits, s_eoff = d_text.clone(), d_toff[: ns + 1].clone(), d_edits.clone(), d_eoff[: ns + 1].clone()
ctx.tokenize(s_text.data_ptr(), s_toff.data_ptr(), ns, nbytes, d_tok.data_ptr(), tcap, d_koff.data_ptr(), d_kst.data_ptr()); ntok = ctx.sync()
d_spans = torch.empty((tcap, 4), dtype=torch.int32, device=dev)
def spans():
    ctx.source_spans(d_tok.data_ptr(), d_koff.data_ptr(), ns, s_edits.data_ptr(), s_eoff.data_ptr(), d_spans.data_ptr(), tcap); return ctx.sync_lines()
arms = {"a": lambda: norm(cu, co), "A": lambda: aligned(cu, co), "b": lambda: norm(mu, mo), "B": lambda: aligned(mu, mo), "s": spans}
for f in arms.values():   # warm-up: tables uploaded, scratch sized, clocks up
    for _ in range(3): f()
assert norm(cu, co) == cbytes and aligned(cu, co) == (cbytes, 0), "clean text must come out as it went in, without edits"
print(f"{kind}: {n} sentences, {cbytes} clean bytes, {mbytes} bytes with 10 % half-/full-width ({aligned(mu, mo)[1]} edits); spans: {ns} sentences, {ntok} records, {nedits} edits")
print(f"{reps} repetitions of {rounds} interleaved rounds, one batch in flight; medians in us")
meds = {k: [] for k in arms}
for r in range(reps):
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
    for k in arms: meds[k].append(float(np.median(times[k])) * 1e6)
    print(f"  rep {r}: " + "  ".join(f"({k}) {meds[k][-1]:.1f}" for k in arms) + f"   A/a {meds['A'][-1] / meds['a'][-1]:.3f}  B/b {meds['B'][-1] / meds['b'][-1]:.3f}")
for k in arms:
    v = np.array(meds[k]); print(f"  ({k}) median of medians {np.median(v):.1f} us, min {v.min():.1f}, max {v.max():.1f}, spread {(v.max() - v.min()) / np.median(v) * 100:.1f} %")
ra, rb = np.array(meds["A"]) / np.array(meds["a"]), np.array(meds["B"]) / np.array(meds["b"])
print(f"  A/a: median {np.median(ra):.3f} (min {ra.min():.3f}, max {ra.max():.3f})   B/b: median {np.median(rb):.3f} (min {rb.min():.3f}, max {rb.max():.3f})")
print(f"  spans: {np.median(meds['s']):.1f} us for {ntok} records of {ns} sentences")
