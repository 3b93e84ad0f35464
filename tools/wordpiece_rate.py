#!/usr/bin/env python
"""The WordPiece ids' rates (kgpu_wordpiece.hip behind the encode entry points) beside the plain encode on cfg 2: 100k sentences, batches of 4096, 8
contexts, the synthetic 392k dictionary with synth.feature_tables, surface field, no filter.  The layout is tools/encode_rate.py's, whose device loop
this file uses.

    python tools/wordpiece_rate.py [--out profiles/experiments/wordpiece_rate.txt] [--no-trace]

Every leg is a child process under its own `timeout`.  A leg exits 0, or 3 when its criterion is not met (the run goes on and ends with 1); any
other status -- an exception, a HIP error, a fault, a time limit -- ends the run with the leg's stderr: nothing more is started on the device.
  host     THE YARDSTICK: a list in which every corpus word is whole (the whole read-out of a count of the corpus).  kgpu_encode_batch on a
           WordPiece handle of that list against the plain handle's -- whose kernels are the plain encode's, untouched --, alternated in one process:
           five windows each, medians and spreads ((max - min) / median).  Criterion: the WordPiece median lies within the plain call's own spread
           of the plain median.  The ids of the two calls are compared as well.
  device   a BERT-like list of 32k entries (specials, the top words, then the corpus's characters c and ##c): the share of multi-piece and [UNK]
           tokens and the ids per token (by Vocab.split_words over the count's read-out, weighted by the counts), and records alone, records +
           plain ragged encode, + WordPiece ragged, + WordPiece padded at width 64: alternated, medians of three; the ratios to records alone.
  trace    rocprofv3 --kernel-trace --stats over a child that runs the device leg once per consumer: microseconds per 4096-sentence batch of
           k_wordpiece_* beside k_encode_* (no threshold)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("KANPYO_SYNTH_CACHE", "/tmp/kanpyo_synth")

import numpy as np  # noqa: E402

import encode_rate as ER  # noqa: E402  (N, BATCH, Q, WIDTH, device_runs)

LIST_SIZE = 32000
SPECIALS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"]


def setup():
    """-> tok, sents, pack_sentences, words handle, the corpus's (word, count) read-out, the packed corpus."""
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    sents = synth.make_corpus(sd, ER.N, 1, "cfg2")
    w = tok.words()
    k = w.counter()
    utf8, offs = pack_sentences(sents)
    k.add_packed(utf8, offs)
    counts = k.most_common()
    k.close()
    return tok, sents, pack_sentences, w, counts, (utf8, offs)


def characters(word):
    starts = [i for i in range(len(word)) if i == 0 or word[i] & 0xC0 != 0x80] + [len(word)]
    return [word[a:b] for a, b in zip(starts, starts[1:])]


def bert_like(counts):
    """Specials, then the characters of the corpus as c and ##c, and the most frequent words in front of them up to LIST_SIZE entries."""
    chars = sorted({c for word, _ in counts for c in characters(word)})
    room = max(LIST_SIZE - len(SPECIALS) - 2 * len(chars), 0)
    head = [word for word, _ in counts if word not in SPECIALS][:room]
    seen = set(SPECIALS) | set(head)
    return SPECIALS + head + [c for c in chars if c not in seen] + [b"##" + c for c in chars if b"##" + c not in seen]


def leg_host(say):
    from kanpyo_amd.vocab import Vocab

    tok, sents, pack_sentences, w, counts, (utf8, offs) = setup()
    words = SPECIALS + [word for word, _ in counts if word not in SPECIALS]
    handles = {"plain": Vocab(w, words, 1), "wordpiece": Vocab(w, words, 1, wordpiece=True)}
    n = ER.N
    outs, ts = {}, {k: [] for k in handles}
    for k, v in handles.items():   # caller-owned arrays, reused; a warm-up call each
        first, _, _ = v.encode_packed(utf8, offs)
        outs[k] = (np.empty(first.size, dtype=first.dtype), np.empty(n + 1, dtype=np.uint64), np.empty(n, dtype=np.uint8))
        v.encode_packed(utf8, offs, out=outs[k])
    equal = all(np.array_equal(a, b) for a, b in zip(outs["plain"], outs["wordpiece"]))
    for _ in range(5):   # alternated in one process
        for k, v in handles.items():
            t0 = time.perf_counter()
            v.encode_packed(utf8, offs, out=outs[k])
            ts[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(x)) for k, x in ts.items()}
    spread = {k: (max(x) - min(x)) / med[k] for k, x in ts.items()}
    say(f"host in / host out, {n} sentences, {int(offs[-1])} input bytes, five windows each, alternated; a list of {len(words)} words in which every corpus word is whole: "
        f"{handles['wordpiece'].info()} {handles['wordpiece'].wordpiece_info()}; ids equal: {equal}")
    for k in handles:
        say(f"  {k:<10} {n / med[k] / 1e6:6.2f} M sentences/s, spread {100 * spread[k]:.1f} %, {outs[k][0].size} ids  (windows: {', '.join(f'{n / x / 1e6:.1f}' for x in ts[k])})")
    ratio = med["wordpiece"] / med["plain"]
    ok = abs(ratio - 1) <= spread["plain"] and equal
    say(f"  criterion: the WordPiece median within the plain call's own spread of the plain median: WordPiece takes {ratio:.3f} x the plain call's time, "
        f"allowed 1 +- {spread['plain']:.3f}: {'met' if ok else 'NOT MET'}")
    return ok


def device_handles(w, counts):
    from kanpyo_amd.vocab import Vocab

    words = bert_like(counts)
    return words, Vocab(w, words, 1), Vocab(w, words, 1, wordpiece=True)


LABEL = {"records": "records alone", "plain": "records + plain ragged encode", "ragged": "records + WordPiece ragged", "padded": f"records + WordPiece padded, width {ER.WIDTH}"}


def leg_device(say):
    tok, sents, pack_sentences, w, counts, _ = setup()
    words, plain, wp = device_handles(w, counts)
    # the shares, by the library's host split over the distinct words, weighted by their counts
    listed = set(words)
    splits = wp.split_words([word for word, _ in counts])
    tokens = sum(c for _, c in counts)
    multi = sum(c for (word, c), s in zip(counts, splits) if len(s) > 1)
    unks = sum(c for (word, c), s in zip(counts, splits) if len(s) == 1 and word not in listed)
    ids = sum(c * len(s) for (_, c), s in zip(counts, splits))
    say(f"BERT-like list of {len(words)} entries: {wp.info()} {wp.wordpiece_info()}")
    say(f"  {tokens} kept tokens: {100 * multi / tokens:.2f} % multi-piece, {100 * unks / tokens:.2f} % [UNK], {ids / tokens:.3f} ids per token")
    cons = {"records": None, "plain": ("ragged", plain), "ragged": ("ragged", wp), "padded": ("padded", wp)}
    out, got = ER.device_runs(tok, sents, pack_sentences, cons, reps=3)
    med = {k: float(np.median(x)) for k, x in out.items()}
    for k in out:
        say(f"device-resident, {LABEL[k]:<40}: {med[k] / 1e6:6.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in out[k])})")
    say("  ratios to records alone: " + ", ".join(f"{k} {med[k] / med['records']:.2f}" for k in ("plain", "ragged", "padded")))
    say(f"  {got['ragged'][0]} tokens; plain: {got['plain'][1]} ids; WordPiece ragged: {got['ragged'][1]} ids")
    return True


def leg_trace_child():
    tok, sents, pack_sentences, w, counts, _ = setup()
    _, plain, wp = device_handles(w, counts)
    ER.device_runs(tok, sents, pack_sentences, {"plain": ("ragged", plain), "ragged": ("ragged", wp), "padded": ("padded", wp)}, reps=1)


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
        if k.startswith(("k_lines_scan", "k_wordpiece_", "k_encode_")):
            c, ns = ks[k]
            say(f"  {k:<18} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    scan = ks["k_lines_scan"][1] / ks["k_lines_scan"][0]   # (shared by the consumers)
    per = {p: sum(ks[f"k_{p}_{s}"][1] / ks[f"k_{p}_{s}"][0] for s in ("len", "write")) + scan for p in ("encode", "wordpiece")}
    say(f"  kernel time per 4096-sentence batch (len + scan + write): plain encode {per['encode'] / 1e3:.1f} us, WordPiece {per['wordpiece'] / 1e3:.1f} us "
        f"(k_wordpiece_write's figure averages the ragged and the padded runs)")
    return True


NOT_MET = 3   # a leg's exit status for "ran through, its criterion is not met"; anything else but 0 is trouble
LEGS = {"host": (leg_host, 500), "device": (leg_device, 500), "trace": (leg_trace, 500)}


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

    lines = [f"# tools/wordpiece_rate.py: cfg 2, {ER.N} sentences, batches of {ER.BATCH}, {ER.Q} contexts; synthetic 392k dictionary + synth.feature_tables; surface field, "
             f"no filter; library {_lib.kernel_source_hash()}"]
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
