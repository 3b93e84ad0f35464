#!/usr/bin/env python
"""The vocabulary ids' rates (kgpu_encode.hip and the encode entry points) beside the wakati render on cfg 2: 100k sentences, batches of 4096, 8
contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter; the vocabulary is the whole read-out of a count of the
same corpus behind <pad> and <unk>.

    python tools/encode_rate.py [--out profiles/experiments/encode_rate.txt] [--no-trace]

Every leg is a child process under its own `timeout`.  A leg exits 0, or 3 when its criterion is not met (the run goes on and ends with 1); any
other status -- an exception, a HIP error, a fault, a time limit -- ends the run with the leg's stderr: nothing more is started on the device.
  host     kgpu_encode_batch against kgpu_tokenize_batch_words, alternated in one process: five windows each, medians and spreads ((max - min) /
           median).  The yardstick is the words call, which writes about 4.5 bytes per token where encode writes 4.  Criterion: encode is not
           slower than words by more than the spread of the words call's own five windows in this run.
  device   records alone, records + words render, records + ragged encode, records + padded encode at width 64: the loop of
           tools/lines_rate.py::device_leg with the consumer as a parameter, alternated, medians of three; the ratios to records alone (no threshold).
  trace    rocprofv3 --kernel-trace --stats over a child that runs the device leg once per consumer: microseconds per 4096-sentence batch of
           k_encode_* beside k_words_* (no threshold)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("KANPYO_SYNTH_CACHE", "/tmp/kanpyo_synth")

import numpy as np  # noqa: E402

N, BATCH, Q, WIDTH = 100_000, 4096, 8, 64


def setup():
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    sents = synth.make_corpus(sd, N, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    utf8, offs = pack_sentences(sents)
    k.add_packed(utf8, offs)
    v = k.vocabulary()
    k.close()
    return tok, sents, pack_sentences, w, v, (utf8, offs)


def device_runs(tok, sents, pack_sentences, consumers, reps):
    """tools/lines_rate.py::device_leg with what reads the records as a parameter: None, ("words", Words), ("ragged", Vocab) or ("padded", Vocab)
    -> {name: [sentences/s]}, {name: (tokens, bytes or ids reported)}."""
    import torch

    from kanpyo_amd.device import DeviceContext

    dev = torch.device("cuda", 0)
    batches = []
    for lo in range(0, len(sents), BATCH):
        u, o = pack_sentences(sents[lo : lo + BATCH])
        n, cap = len(o) - 1, int(o[-1]) + len(o)
        batches.append((torch.from_numpy(u.copy()).to(dev), torch.from_numpy(o.astype(np.int64)).to(dev), n, int(o[-1]), cap))
    ctxs = [DeviceContext(tok) for _ in range(Q)]
    cap = max(b[4] for b in batches)
    bufs = [(torch.empty((cap, 6), dtype=torch.int32, device=dev), torch.empty(BATCH + 1, dtype=torch.int64, device=dev), torch.empty(BATCH, dtype=torch.uint8, device=dev),
             torch.empty(32 << 20, dtype=torch.uint8, device=dev), torch.empty(BATCH + 1, dtype=torch.int64, device=dev)) for _ in range(Q)]
    LAG = Q - 2
    counts = {}

    def run(name, consumer):
        tokens = out = 0
        nb = len(batches)
        t0 = time.perf_counter()
        for i in range(nb + LAG):
            if i < nb:
                k = i % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                out += c.sync_lines()
                du, do, n, total, bcap = batches[i]
                c.tokenize(du.data_ptr(), do.data_ptr(), n, total, dt.data_ptr(), bcap, dto.data_ptr(), dst.data_ptr())
            j = i - LAG
            if j >= 0:
                k = j % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                tokens += c.sync()
                du, do, n, total, bcap = batches[j]
                if consumer is None:
                    continue
                kind, h = consumer
                if kind == "words":
                    c.format_words(h, du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), dtext.data_ptr(), dtext.numel(), dtexto.data_ptr())
                else:
                    c.encode(h, du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), dtext.data_ptr(), dtext.numel() // 4, dtexto.data_ptr(),
                             width=WIDTH if kind == "padded" else 0, pad_id=0)
        for c in ctxs:
            out += c.sync_lines()
        counts[name] = (tokens, out)
        return len(sents) / (time.perf_counter() - t0)

    res = {name: [] for name in consumers}
    for name, r in consumers.items():
        run(name, r)   # warm-up
    for _ in range(reps):   # alternated
        for name, r in consumers.items():
            res[name].append(run(name, r))
    for c in ctxs:
        c.close()
    return res, counts


def consumers_of(w, v):
    return {"records": None, "words": ("words", w), "ragged": ("ragged", v), "padded": ("padded", v)}


LABEL = {"records": "records alone", "words": "records + words render", "ragged": "records + ragged encode", "padded": f"records + padded encode, width {WIDTH}"}


def leg_device(say):
    tok, sents, pack_sentences, w, v, _ = setup()
    out, counts = device_runs(tok, sents, pack_sentences, consumers_of(w, v), reps=3)
    med = {k: float(np.median(x)) for k, x in out.items()}
    for k in out:
        say(f"device-resident, {LABEL[k]:<36}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    say("  ratios to records alone: " + ", ".join(f"{k} {med[k] / med['records']:.2f}" for k in ("words", "ragged", "padded")))
    say(f"  {counts['ragged'][0]} tokens; words: {counts['words'][1]} bytes of text; ragged: {counts['ragged'][1]} ids = {4 * counts['ragged'][1]} bytes; "
        f"padded: {N} x {WIDTH} ids = {4 * N * WIDTH} bytes; vocabulary: {v.info()}")
    return True


def leg_trace_child():
    tok, sents, pack_sentences, w, v, _ = setup()
    cons = consumers_of(w, v)
    del cons["records"]
    device_runs(tok, sents, pack_sentences, cons, reps=1)


def leg_trace(say):
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--leg", "trace-child"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        ks = {}
        with open(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
            for row in csv.DictReader(f):
                ks[row["Name"].split("(")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    for k in sorted(ks):
        if k.startswith(("k_lines_scan", "k_words_", "k_encode_")):
            c, ns = ks[k]
            say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = ks["k_lines_scan"][1] / ks["k_lines_scan"][0]   # (shared by the three consumers)
    per = {p: sum(ks[f"k_{p}_{s}"][1] / ks[f"k_{p}_{s}"][0] for s in ("len", "write")) + scan for p in ("words", "encode")}
    say(f"  kernel time per 4096-sentence batch (len + scan + write): words {per['words'] / 1e3:.1f} us, encode {per['encode'] / 1e3:.1f} us "
        f"(k_encode_write's figure averages the ragged and the padded runs)")
    return True


def leg_host(say):
    tok, sents, pack_sentences, w, v, (utf8, offs) = setup()
    calls = {"words": w.render_packed, "encode": v.encode_packed}
    outs, sizes, ts = {}, {}, {k: [] for k in calls}
    for k, f in calls.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = f(utf8, offs)
        sizes[k] = first.size
        outs[k] = (np.empty(first.size, dtype=first.dtype), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
        f(utf8, offs, out=outs[k])
    for _ in range(5):   # alternated in one process
        for k, f in calls.items():
            t0 = time.perf_counter()
            f(utf8, offs, out=outs[k])
            ts[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(x)) for k, x in ts.items()}
    spread = {k: (max(x) - min(x)) / med[k] for k, x in ts.items()}
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


NOT_MET = 3   # a leg's exit status for "ran through, its criterion is not met"; anything else but 0 is trouble
LEGS = {"host": (leg_host, 500), "device": (leg_device, 400), "trace": (leg_trace, 500)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.leg == "trace-child":
        leg_trace_child()
        return
    if args.leg:
        ok = LEGS[args.leg][0](lambda s: print(s, flush=True))
        sys.exit(0 if ok else NOT_MET)
    from kanpyo_amd import _lib

    lines = [f"# tools/encode_rate.py: cfg 2, {N} sentences, batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
             f"no filter; vocabulary = <pad>, <unk> and the whole read-out of a count of the same corpus; library {_lib.kernel_source_hash()}"]
    print(lines[0], flush=True)
    ok = True
    for name, (_, limit) in LEGS.items():
        if name == "trace" and args.no_trace:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode not in (0, NOT_MET):   # an exception, a fault, an abort or a time limit: nothing more runs on the device
            lines.append(f"leg {name} ended with status {r.returncode}; its stderr ends: {r.stderr[-3000:]}")
            print(lines[-1], flush=True)
            ok = False
            break
        ok = ok and r.returncode == 0
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
