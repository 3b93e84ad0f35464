#!/usr/bin/env python
"""The text from ids' rate (kgpu_decode.hip) beside the wakati render (kgpu_words.hip) of the same batch in the same build: ONE batch of 4096 cfg 2
sentences, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.  The vocabulary is the whole read-out of a count of the
batch behind <pad> and <unk>: every word is listed, so decode writes the bytes the words render writes minus the newlines (checked here), and reads 4
bytes per element where the render reads a 24-byte record.

    python tools/decode_rate.py [--out profiles/experiments/decode_rate.txt] [--no-trace]

Every leg is a child process under its own `timeout`.  A leg exits 0; any other status -- an exception, a HIP error, a fault, a time limit -- ends
the run with the leg's stderr: nothing more is started on the device.
  device   the records and the ids stay in HBM; a window is ITERS enqueue + sync_lines pairs of one consumer on one context; five windows each,
           alternated; medians, spreads ((max - min) / median) and the ratio decode / words of the medians (no threshold: none has been measured before).
  trace    rocprofv3 --kernel-trace --stats over a child that runs each consumer ITERS times: microseconds per batch of k_decode_* beside k_words_*."""
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

BATCH, ITERS, WINDOWS = 4096, 2000, 5   # (a window is a few tenths of a second)


def setup():
    """-> (context, {name: enqueue()}, facts): the batch tokenized and encoded once, both consumers' buffers in HBM."""
    import torch  # (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    sents = synth.make_corpus(sd, BATCH, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    utf8, offs = pack_sentences(sents)
    k.add_packed(utf8, offs)
    v = k.vocabulary()
    k.close()
    dev = torch.device("cuda", 0)
    n, total = len(offs) - 1, int(offs[-1])
    du = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    do = torch.from_numpy(offs.astype(np.int64)).to(dev)
    cap = total + n + 64
    dt, dto, dst = torch.empty((cap, 6), dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    ids, ioff = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    text_w, toff_w = torch.empty(16 << 20, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    text_d, toff_d, st_d = torch.empty(16 << 20, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c = DeviceContext(tok)
    c.tokenize(du.data_ptr(), do.data_ptr(), n, total, dt.data_ptr(), cap, dto.data_ptr(), dst.data_ptr())
    tokens = c.sync()
    c.encode(v, du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), ids.data_ptr(), cap, ioff.data_ptr())
    n_ids = c.sync_lines()
    calls = {
        "words": lambda: c.format_words(w, du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), text_w.data_ptr(), text_w.numel(), toff_w.data_ptr()),
        "decode": lambda: c.decode(v, ids.data_ptr(), ioff.data_ptr(), n, text_d.data_ptr(), text_d.numel(), toff_d.data_ptr(), st_d.data_ptr()),
    }
    size = {}
    for name, f in calls.items():   # once each: the first decode uploads the handle's id -> word table
        f()
        size[name] = c.sync_lines()
    # every word is listed: the decoded lines are the rendered lines without their newlines
    a, ao = text_w[: size["words"]].cpu().numpy().tobytes(), toff_w.cpu().tolist()
    b, bo = text_d[: size["decode"]].cpu().numpy().tobytes(), toff_d.cpu().tolist()
    same = all(a[ao[i] : ao[i + 1] - 1] == b[bo[i] : bo[i + 1]] for i in range(n)) and not bool(st_d.any())
    facts = dict(n=n, input_bytes=total, tokens=tokens, ids=n_ids, words_bytes=size["words"], decode_bytes=size["decode"], same=same, vocabulary=len(v.words))
    keep = (tok, w, v, du, do, dt, dto, dst, ids, ioff, text_w, toff_w, text_d, toff_d, st_d)
    return c, calls, facts, keep


def window(c, f):
    t0 = time.perf_counter()
    for _ in range(ITERS):
        f()
        c.sync_lines()
    return (time.perf_counter() - t0) / ITERS


def leg_device(say):
    c, calls, facts, _keep = setup()
    say(f"one batch: {facts['n']} sentences, {facts['input_bytes']} input bytes, {facts['tokens']} records, {facts['ids']} ids, vocabulary of {facts['vocabulary']} words; "
        f"words render {facts['words_bytes']} bytes, decode {facts['decode_bytes']} bytes; decoded lines == rendered lines minus the newline: {facts['same']}")
    if not facts["same"] or facts["decode_bytes"] != facts["words_bytes"] - facts["n"]:
        raise RuntimeError("the decoded lines are not the rendered lines")
    ts = {k: [] for k in calls}
    for k, f in calls.items():
        window(c, f)   # warm-up
    for _ in range(WINDOWS):   # alternated
        for k, f in calls.items():
            ts[k].append(window(c, f))
    med = {k: float(np.median(x)) for k, x in ts.items()}
    spread = {k: (max(x) - min(x)) / med[k] for k, x in ts.items()}
    for k in calls:
        say(f"  {k:<7} {med[k] * 1e6:7.1f} us per batch (enqueue + sync, {ITERS} per window), spread {100 * spread[k]:.1f} %  (windows: {', '.join(f'{x * 1e6:.1f}' for x in ts[k])})")
    say(f"  ratio decode / words of the medians: {med['decode'] / med['words']:.3f}  (the words render's own spread: {100 * spread['words']:.1f} %)")
    return True


def leg_trace_child():
    c, calls, _, _keep = setup()
    for f in calls.values():
        for _ in range(ITERS):
            f()
            c.sync_lines()


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
        if k.startswith(("k_lines_scan", "k_words_", "k_decode_")):
            n, ns = ks[k]
            say(f"  {k:<16} {n} calls, {ns / 1e3 / n:8.1f} us per call")
    scan = ks["k_lines_scan"][1] / ks["k_lines_scan"][0]   # (shared by the consumers)
    per = {p: sum(ks[f"k_{p}_{s}"][1] / ks[f"k_{p}_{s}"][0] for s in ("len", "write")) + scan for p in ("words", "decode")}
    say(f"  kernel time per {BATCH}-sentence batch (len + scan + write): words {per['words'] / 1e3:.1f} us, decode {per['decode'] / 1e3:.1f} us, ratio {per['decode'] / per['words']:.3f}")
    return True


LEGS = {"device": (leg_device, 400), "trace": (leg_trace, 500)}


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
        LEGS[args.leg][0](lambda s: print(s, flush=True))
        return
    from kanpyo_amd import _lib

    lines = [f"# tools/decode_rate.py: cfg 2, one batch of {BATCH} sentences, one context; synthetic 392k dictionary + synth.feature_tables; surface field, no filter; "
             f"vocabulary = <pad>, <unk> and the whole read-out of a count of the batch; library {_lib.kernel_source_hash()}"]
    print(lines[0], flush=True)
    ok = True
    for name, (_, limit) in LEGS.items():
        if name == "trace" and args.no_trace:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:   # an exception, a fault, an abort or a time limit: nothing more runs on the device
            lines.append(f"leg {name} ended with status {r.returncode}; its stderr ends: {r.stderr[-3000:]}")
            print(lines[-1], flush=True)
            ok = False
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
