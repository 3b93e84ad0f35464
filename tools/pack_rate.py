#!/usr/bin/env python
"""The model inputs' cost (kgpu_pack.hip, include/kanpyo_gpu.h "model inputs") beside the ragged encode step it follows, on the synthetic 392k dictionary
with a WordPiece list of every character and ##character of the corpus, [CLS] / [SEP] added by the vocabulary:
  cfg 2    16 384 sentences of about 40 characters, singles, max_length 64 and max_length 512 (one row each: the cost of the padding)
  cfg 5    256 documents of 2048 characters, singles, max_length 512, stride 128 (overlapping windows)
each without and with spans and token indices.

    python tools/pack_rate.py [--out profiles/experiments/pack_rate.txt]

The measuring leg is a child process under its own `timeout`; any status but 0 ends the run with the leg's stderr.  Method (tools/encode_spans_timing.py's):
ONE context with ONE batch in flight, device-resident records tokenized once outside the timing, the two arms -- kgpu_encode_device[_spans] (ragged) and
kgpu_pack_device on what it wrote -- interleaved in one process, five repetitions of 15 rounds, a host clock around enqueue + kgpu_ctx_sync_lines; the
median of the five medians in us and the spread of the medians.  Both arms are three launches and one wait: a call of a few tens of microseconds is mostly
that.  Two figures per row: the pack's time over the encode's, and the pack's bytes -- read (the ids it copies, with spans 20 bytes more per element, and the
offsets) plus written (12 bytes per slot, 32 with spans, and the row offsets and status) -- over its time, beside the 6.29 TB/s copy rate DESIGN.md uses."""
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

COPY_RATE = 6.29e12   # the chip's measured copy rate, bytes/s
REPS, ROUNDS = 5, 15
CASES = [("cfg 2 x 16384, max_length 64", "cfg2", 16384, 64, 0), ("cfg 2 x 16384, max_length 512", "cfg2", 16384, 512, 0),
         ("cfg 5 (2048 characters) x 256, max_length 512, stride 128", "cfg5", 256, 512, 128)]


def leg(say, only=None):
    """only = (case index, with spans): that one arm pair alone (the trace's child)."""
    import torch

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.pack import pack_opts
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    for ci, (label, kind, n, ML, stride) in enumerate(CASES):
        if only is not None and only[0] != ci:
            continue
        sents = synth.make_corpus(sd, n, 1, kind)
        chars = sorted({c for s in sents for c in s})
        vocab = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"] + [c.encode() for c in chars] + [b"##" + c.encode() for c in chars]
        v = tok.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
        utf8, offs = pack_sentences(sents)
        total = int(offs[-1])
        d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        cap = total + n + 64
        d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
        d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, total, d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
        ctx.sync()
        id_cap = total + 2 * n + 64   # (a piece is a character at least)
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
                args = (v, d_utf8.data_ptr(), d_off.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_ids.data_ptr(), id_cap, d_ioff.data_ptr())
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
            med = {"encode": [], "pack": []}
            for _ in range(REPS):
                ts = {"encode": [], "pack": []}
                for _ in range(ROUNDS):   # interleaved
                    for name, f in (("encode", encode), ("pack", pack)):
                        t0 = time.perf_counter()
                        f()
                        ts[name].append(time.perf_counter() - t0)
                for k in ts:
                    med[k].append(float(np.median(ts[k])))
            m = {k: float(np.median(x)) for k, x in med.items()}
            sp = {k: (max(x) - min(x)) / m[k] for k, x in med.items()}
            rate = moved / m["pack"]
            say(f"{label}, {'with' if with_spans else 'no'} spans: {n_ids} ids -> {R} rows; ragged encode {m['encode'] * 1e6:8.1f} us ({100 * sp['encode']:.1f} %), "
                f"pack {m['pack'] * 1e6:8.1f} us ({100 * sp['pack']:.1f} %), pack / encode {m['pack'] / m['encode']:.3f}; pack moves {moved} bytes: "
                f"{rate / 1e9:7.1f} GB/s = {100 * rate / COPY_RATE:.1f} % of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
        v.close()
    ctx.close()
    return True


def trace(say):
    """rocprofv3 --kernel-trace --stats over a child that runs ONE arm pair (the largest case, cfg 2 at max_length 512): the kernels' own time per call,
    without the launches' and the wait's share of the host clock."""
    ci = 1
    for with_spans in (0, 1):
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                   sys.executable, os.path.abspath(__file__), "--leg", "--only", f"{ci}:{with_spans}"]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
            ks = {}
            with open(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
                for row in csv.DictReader(f):
                    ks[row["Name"].split("(")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
        say(f"kernel trace, {CASES[ci][0]}, {'with' if with_spans else 'no'} spans: " + ", ".join(
            f"{k} {ns / 1e3 / c:.1f} us x {c}" for k, (c, ns) in sorted(ks.items()) if k.startswith(("k_pack_", "k_lines_scan", "k_wordpiece_"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.leg:
        leg(lambda s: print(s, flush=True), None if args.only is None else (int(args.only.split(":")[0]), args.only.endswith(":1")))
        return
    from kanpyo_amd import _lib

    lines = [f"# tools/pack_rate.py: one context, one batch in flight, {REPS} x {ROUNDS} rounds interleaved, host clock around enqueue + sync; synthetic 392k dictionary, "
             f"WordPiece list of every character and ##character; library {_lib.kernel_source_hash()}"]
    print(lines[0], flush=True)
    r = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--leg"], capture_output=True, text=True, cwd=ROOT)
    print(r.stdout, end="", flush=True)
    lines += r.stdout.splitlines()
    if r.returncode != 0:   # an exception, a fault, an abort or a time limit: nothing more runs on the device
        lines.append(f"the leg ended with status {r.returncode}; its stderr ends: {r.stderr[-3000:]}")
        print(lines[-1], flush=True)
    if r.returncode == 0 and not args.no_trace:   # (only behind a leg that ran through: nothing more is started on the device after a failure)
        def say(x):
            print(x, flush=True)
            lines.append(x)

        try:
            trace(say)
        except RuntimeError as e:
            say(str(e))
            r.returncode = 1
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
