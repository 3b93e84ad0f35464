#!/usr/bin/env python
"""What the normaliser costs beside the tokenizer it feeds (python tools/normalize_timing.py [cfg2|cfg5] [n] [rounds]): on device-resident input,
interleaved in one process, (a) kgpu_normalize_device alone on clean text, (b) the same with 10 % of the characters half-width or full-width,
(c) kgpu_tokenize_device alone on the clean batch.  Prints GB/s of input for (a) and (b), and (a) / (c); medians and minima over the rounds.
One context, one batch in flight: the latency of the three launches, not what several contexts overlap to."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from kanpyo_amd import Tokenizer, synth
from kanpyo_amd.device import DeviceContext
from kanpyo_amd.tokenizer import pack_sentences
kind = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
n = int(sys.argv[2]) if len(sys.argv) > 2 else (16384 if kind == "cfg2" else 256)
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 15
HALF = "ｱｲｳｴｵｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾅﾆﾇﾈﾉ"
FULL = "ＡＢＣＤＥＦＧＨＩＪ０１２３４５６７８９"
def dirty(s, rng):   # every tenth character, on average, becomes a half-width kana or a full-width letter or digit
    pool = HALF + FULL
    return "".join(pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.1 else c for c in s)
from kanpyo_amd import normalize_host
sd = synth.build_dict(); clean = [normalize_host(x).decode() for x in synth.make_corpus(sd, n, 1, kind)]   # (the synthetic corpus holds a few code points NFKC changes: clean means none)
rng = np.random.default_rng(5); mixed = [dirty(s, rng) for s in clean]
tok = Tokenizer(sd.dict); dev = torch.device("cuda", 0); ctx = DeviceContext(tok)
def resident(sents):
    utf8, offs = pack_sentences(sents)
    return torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev), int(offs[-1])
cu, co, cbytes = resident(clean); mu, mo, mbytes = resident(mixed)
ncap = 3 * max(cbytes, mbytes) + 64
d_text = torch.empty(ncap + 16, dtype=torch.uint8, device=dev); d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev); d_st = torch.empty(n, dtype=torch.uint8, device=dev)
tcap = cbytes + n + 64
d_tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev); d_koff = torch.empty(n + 1, dtype=torch.int64, device=dev); d_kst = torch.empty(n, dtype=torch.uint8, device=dev)
def norm(u, o):
    ctx.normalize(u.data_ptr(), o.data_ptr(), n, d_text.data_ptr(), ncap, d_toff.data_ptr(), d_st.data_ptr(), "NFKC"); return ctx.sync_normalize()
def tokenize():
    ctx.tokenize(cu.data_ptr(), co.data_ptr(), n, cbytes, d_tok.data_ptr(), tcap, d_koff.data_ptr(), d_kst.data_ptr()); return ctx.sync()
arms = {"a": lambda: norm(cu, co), "b": lambda: norm(mu, mo), "c": tokenize}
for f in arms.values():   # warm-up: tables uploaded, scratch sized, clocks up
    for _ in range(3): f()
assert norm(cu, co) == cbytes, "clean text must come out as it went in"
times = {k: [] for k in arms}
for _ in range(rounds):
    for k, f in arms.items():
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
med = {k: float(np.median(v)) for k, v in times.items()}; low = {k: float(np.min(v)) for k, v in times.items()}
print(f"{kind}: {n} sentences, {cbytes} clean bytes, {mbytes} bytes with 10 % half-/full-width; {rounds} interleaved rounds, one batch in flight")
print(f"  (a) normalise clean: median {med['a'] * 1e6:.0f} us (min {low['a'] * 1e6:.0f}) = {cbytes / med['a'] / 1e9:.2f} GB/s")
print(f"  (b) normalise mixed: median {med['b'] * 1e6:.0f} us (min {low['b'] * 1e6:.0f}) = {mbytes / med['b'] / 1e9:.2f} GB/s")
print(f"  (c) tokenize clean:  median {med['c'] * 1e6:.0f} us (min {low['c'] * 1e6:.0f})")
print(f"  (a) / (c) = {med['a'] / med['c']:.3f}   (b) / (c) = {med['b'] / med['c']:.3f}")
