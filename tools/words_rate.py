#!/usr/bin/env python
"""The wakati output's rates (kgpu_words.hip and the words entry points) beside the `kanpyo tokenize` lines on cfg 2: 100k sentences, batches of
4096, 8 contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.

    python tools/words_rate.py [--out profiles/experiments/words_rate.txt]

Every leg is a child process under its own `timeout`.  A leg exits 0, or 3 when a requirement is not met (the run goes on and ends with 1); any
other status -- an exception, a HIP error, a fault, a time limit -- ends the run with the leg's stderr: nothing more is started on the device.
  host     kgpu_tokenize_batch_words against kgpu_tokenize_batch_lines, alternated in one process: five windows each, medians, sentences/s and
           GB/s of text.  Required: the words median is not below the lines median of the same run.  Then the DROP [助詞, 助動詞, 記号] and the
           field 7 handles, for what the table lookup and the compaction cost (no threshold).
  device   records alone, records + lines render, records + words render: the loop of tools/lines_rate.py::device_leg with the render as a
           parameter, alternated.  Required: the words ratio (to records alone) is above the lines ratio of the same run.
  trace    rocprofv3 --kernel-trace --stats over a child that runs the device leg once per render: microseconds per 4096-sentence batch of
           k_words_* beside k_lines_*, and the bytes moved per token (no threshold)."""
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

N, BATCH, Q = 100_000, 4096, 8
POS_DROP = ("助詞", "助動詞", "記号")


def setup():
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return tok, synth.make_corpus(sd, N, 1, "cfg2"), pack_sentences


def device_runs(tok, sents, pack_sentences, renders, reps):
    """tools/lines_rate.py::device_leg with the render as a parameter (None, "lines" or a Words handle) -> {name: [sentences/s]}, {name: (tokens, text bytes)}."""
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

    def run(name, render):
        tokens = text = 0
        nb = len(batches)
        t0 = time.perf_counter()
        for i in range(nb + LAG):
            if i < nb:
                k = i % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                text += c.sync_lines()
                du, do, n, total, bcap = batches[i]
                c.tokenize(du.data_ptr(), do.data_ptr(), n, total, dt.data_ptr(), bcap, dto.data_ptr(), dst.data_ptr())
            j = i - LAG
            if j >= 0:
                k = j % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                tokens += c.sync()
                du, do, n, total, bcap = batches[j]
                if render == "lines":
                    c.format_lines(du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), dtext.data_ptr(), dtext.numel(), dtexto.data_ptr())
                elif render is not None:
                    c.format_words(render, du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), dtext.data_ptr(), dtext.numel(), dtexto.data_ptr())
        for c in ctxs:
            text += c.sync_lines()
        counts[name] = (tokens, text)
        return len(sents) / (time.perf_counter() - t0)

    out = {name: [] for name in renders}
    for name, r in renders.items():
        run(name, r)   # warm-up
    for _ in range(reps):   # alternated
        for name, r in renders.items():
            out[name].append(run(name, r))
    for c in ctxs:
        c.close()
    return out, counts


def leg_device(say):
    tok, sents, pack_sentences = setup()
    w = tok.words()
    out, counts = device_runs(tok, sents, pack_sentences, {"records": None, "lines": "lines", "words": w}, reps=3)
    med = {k: float(np.median(v)) for k, v in out.items()}
    for k in ("records", "lines", "words"):
        say(f"device-resident, {'records alone' if k == 'records' else 'records + ' + k + ' render':<24}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    rl, rw = med["lines"] / med["records"], med["words"] / med["records"]
    tokens, text = counts["words"]
    say(f"  lines ratio {rl:.2f}, words ratio {rw:.2f} of records alone; required: words above lines: {'met' if rw > rl else 'NOT MET'}")
    say(f"  words: {tokens} tokens, {text} bytes of text: {text / N:.0f} bytes per sentence, {text / tokens:.2f} bytes per token (lines: {counts['lines'][1] / counts['lines'][0]:.1f})")
    return rw > rl


def leg_trace_child():
    tok, sents, pack_sentences = setup()
    _, counts = device_runs(tok, sents, pack_sentences, {"lines": "lines", "words": tok.words()}, reps=1)
    print(f"COUNTS {counts['words'][0]} {counts['lines'][1]} {counts['words'][1]} {sum(len(s.encode()) for s in sents)}", flush=True)


def leg_trace(say):
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--leg", "trace-child"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
        tokens, text_lines, text_words, in_bytes = (int(x) for x in [ln for ln in r.stdout.splitlines() if ln.startswith("COUNTS ")][-1].split()[1:])
        ks = {}
        with open(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
            for row in csv.DictReader(f):
                ks[row["Name"].split("(")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    # the scan is shared: its calls are both renders', half each (warm-up + one run per render)
    for k in sorted(ks):
        if k.startswith("k_lines_") or k.startswith("k_words_"):
            c, ns = ks[k]
            say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = ks["k_lines_scan"][1] / ks["k_lines_scan"][0]
    per = {p: sum(ks[f"k_{p}_{s}"][1] / ks[f"k_{p}_{s}"][0] for s in ("len", "write")) + scan for p in ("lines", "words")}
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
    tok, sents, pack_sentences = setup()
    utf8, offs = pack_sentences(sents)
    handles = {"words": tok.words(), "words, DROP 助詞 助動詞 記号": tok.words(drop=POS_DROP), "words, field 7": tok.words(field=7)}
    calls = {"lines": tok.tokenize_lines_packed}
    calls.update({k: h.render_packed for k, h in handles.items()})
    outs, sizes, ts = {}, {}, {k: [] for k in calls}
    for k, f in calls.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = f(utf8, offs)
        sizes[k] = first.size
        outs[k] = (np.empty(first.size, dtype=np.uint8), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
        f(utf8, offs, out=outs[k])
    for _ in range(5):   # alternated in one process
        for k, f in calls.items():
            t0 = time.perf_counter()
            f(utf8, offs, out=outs[k])
            ts[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    say(f"host in / text out, {N} sentences, {int(offs[-1])} input bytes, five windows each, alternated:")
    for k in calls:
        say(f"  {k:<30} {N / med[k] / 1e6:6.2f} M sentences/s, {sizes[k] / med[k] / 1e9:5.2f} GB/s of text, {sizes[k]} bytes = {sizes[k] / int(offs[-1]):.2f} per input byte"
            f"  (windows: {', '.join(f'{N / x / 1e6:.1f}' for x in ts[k])})")
    ok = med["words"] <= med["lines"]
    say(f"  required: the words median is not below the lines median: {N / med['words'] / 1e6:.2f} vs {N / med['lines'] / 1e6:.2f} M sentences/s = "
        f"{med['lines'] / med['words']:.2f} x: {'met' if ok else 'NOT MET'}")
    return ok


NOT_MET = 3   # a leg's exit status for "ran through, a requirement is not met"; anything else but 0 is trouble
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

    lines = [f"# tools/words_rate.py: cfg 2, {N} sentences, batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
             f"no filter unless named; library {_lib.kernel_source_hash()}"]
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
