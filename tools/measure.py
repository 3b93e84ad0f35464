"""The harness of the measuring tools (tools/*_rate.py, tools/*_timing.py, the parent loop of tools/ablate.py): how a figure is taken, once.

Steps and legs.  Whatever uses the device is a child process under `timeout -k 10 <limit>`, started by step() and by nothing else.  A tool is a dictionary
of legs {name: (function, limit in seconds)}: its parent process opens no device, prints a header and runs `python <tool> --leg <name>` leg by leg.  A leg
exits 0, or NOT_MET when it ran through and what it requires does not hold (the run goes on and ends with 1); any other status -- an exception, a HIP
error, a fault, an abort, a time limit -- is recorded with the end of the leg's stderr and ends the run with 1: nothing more is started on the device.
Kernel traces.  trace() runs a child of the tool under rocprofv3 --kernel-trace and returns its rows under kernel_name()'s short names.
Timing.  time.perf_counter on the host; summary() is the median and (max - min) / median; windows(), interleaved() and alternated() are the three ways the
arms of a comparison share a process, pipelined() the loop that keeps Q contexts busy.
Set-up.  The synthetic dictionary's tokenizer, one batch resident in HBM, a corpus cut into batches for pipelined(), and the half-/full-width text of
the normaliser's tools.

Importing this file needs neither a GPU nor torch: what needs them imports them where it is used."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("KANPYO_SYNTH_CACHE", "/tmp/kanpyo_synth")

NOT_MET = 3   # a leg's exit status for "ran through, a requirement is not met"; anything else but 0 is trouble
CARRY = "CARRY "


# ---- steps and legs

def step(argv, limit, cwd=ROOT, stdin=None, text=True):
    """One child process that may use the device: `timeout -k 10 <limit> <argv>` -> (status, stdout, the end of stderr).
    stdin is None, an open file, or what the child is to read."""
    import subprocess

    kw = {"stdin": stdin} if hasattr(stdin, "fileno") else {"input": stdin}
    r = subprocess.run(["timeout", "-k", "10", str(limit), *argv], capture_output=True, text=text, cwd=cwd, **kw)
    return r.returncode, r.stdout, r.stderr[-3000:]


def say(s):
    print(s, flush=True)


def carry(**facts):
    """From a leg: figures a later leg needs.  The parent neither prints nor keeps them; it hands them to every later leg on its stdin."""
    say(CARRY + json.dumps(facts))


def carried():
    """In a later leg: what the legs before it gave to carry().  It reads stdin to its end: the parent gives every leg a pipe, empty for the first; a
    leg started by hand (`--leg <name>`) waits for the figures there, one JSON object per line, then end of file."""
    out = {}
    for ln in sys.stdin.read().splitlines():
        out.update(json.loads(ln))
    return out


def run_legs(tool, legs, header=None, out=None, skip=(), leg_args=(), headings=False):
    """The parent's side -> the tool's exit status.  headings: a `[leg]` line ahead of each leg's lines in the --out file."""
    lines = [] if header is None else [header]
    if header is not None:
        say(header)
    status, facts = 0, ""
    for name, (_, limit) in legs.items():
        if name in skip:
            continue
        if headings:
            lines.append(f"[{name}]")
        rc, stdout, err = step([sys.executable, os.path.abspath(tool), "--leg", name, *leg_args], limit, stdin=facts)
        for ln in stdout.splitlines():
            if ln.startswith(CARRY):
                facts += ln[len(CARRY):] + "\n"
            else:
                say(ln)
                lines.append(ln)
        if rc not in (0, NOT_MET):   # an exception, a fault, an abort or a time limit: nothing more runs on the device
            lines.append(f"leg {name} ended with status {rc}; its stderr ends: {err}")
            say(lines[-1])
            status = 1
            break
        if rc == NOT_MET:
            status = 1
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


def parser(doc, no_trace=False):
    """--out, the hidden --leg and, where the tool has a trace leg, --no-trace."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    if no_trace:
        ap.add_argument("--no-trace", action="store_true")
    return ap


def main(tool, args, legs, header=None, children=None, **kw):
    """Behind the tool's parser.  `--leg <name>` runs that leg here, or one of `children` (the plain programs that trace() profiles); without
    --leg this is the parent.  header is a function, called in the parent alone."""
    if args.leg in (children or {}):
        children[args.leg]()
        return
    if args.leg:
        sys.exit(0 if legs[args.leg][0](say) else NOT_MET)
    sys.exit(run_legs(tool, legs, header() if header else None, out=args.out, **kw))


def library_hash():
    from kanpyo_amd import _lib   # (works without a device)

    return _lib.kernel_source_hash()


# ---- kernel traces

def kernel_name(full):
    """`void kgpu::k_x<kgpu::Foo, 2>(kgpu::A)` -> `k_x<kgpu::Foo, 2>`: a kernel of namespace kgpu or kgpu::dev without `void `, namespace and
    parameter list, with its template arguments.  Any other name (torch's, the runtime's) is returned as it is."""
    s = full[5:] if full.startswith("void ") else full
    for ns in ("kgpu::dev::", "kgpu::"):
        if s.startswith(ns):
            s = s[len(ns):]
            break
    else:
        return full
    depth = 0
    for i, ch in enumerate(s):   # the parameter list opens at the first "(" outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def _rows(d, pattern):
    paths = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    if not paths:
        raise RuntimeError(f"no {pattern} under {d}")
    for path in paths:
        with open(path, newline="") as f:
            yield from csv.DictReader(f)


def read_stats(d):
    """The *kernel_stats.csv under d -> {kernel_name: (calls, total ns)}; rows that share a name are summed."""
    out = {}
    for row in _rows(d, "*kernel_stats.csv"):
        k = kernel_name(row["Name"])
        c, ns = out.get(k, (0, 0.0))
        out[k] = (c + int(row["Calls"]), ns + float(row["TotalDurationNs"]))
    return out


def per_call(ks, fn):
    """ns per call of the kernel function fn in read_stats()'s rows, over its instantiations: `fn` itself and every `fn<...>`."""
    rows = [v for k, v in ks.items() if k == fn or k.startswith(fn + "<")]
    if not rows:
        raise KeyError(f"{fn}: not in the trace; kernels seen: {sorted(ks)}")
    return sum(ns for _, ns in rows) / sum(c for c, _ in rows)


def read_dispatches(d):
    """The *kernel_trace.csv under d -> {kernel_name: [ns of each dispatch, in start order]}."""
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), kernel_name(r["Kernel_Name"])) for r in _rows(d, "*kernel_trace.csv"))
    out = {}
    for _, ns, k in rows:
        out.setdefault(k, []).append(ns)
    return out


def trace(tool, child_args, limit, stats=True):
    """`python <tool> <child_args>` under rocprofv3 --kernel-trace, in a step of its own -> (the child's stdout, read_stats() of the run, or
    read_dispatches() of it with stats=False).  Kernel tracing alone: no other tracing and no counters go with it."""
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        argv = ["rocprofv3", "--kernel-trace", *(["--stats"] if stats else []), "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(tool), *child_args]
        rc, stdout, err = step(argv, limit, cwd=tmp)
        if rc != 0:
            raise RuntimeError(f"rocprofv3 run failed ({rc}): {err}")
        return stdout, (read_stats if stats else read_dispatches)(tmp)


# ---- timing

def summary(xs):
    """-> median, (max - min) / median."""
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


def windows(arms, iters, n=5, clock=time.perf_counter):
    """{arm: call} -> {arm: [seconds per call of each window]}: a window is `iters` calls; one untimed window per arm, then n rounds of one window per arm."""
    def window(f):
        t0 = clock()
        for _ in range(iters):
            f()
        return (clock() - t0) / iters

    for f in arms.values():
        window(f)
    ts = {k: [] for k in arms}
    for _ in range(n):
        for k, f in arms.items():
            ts[k].append(window(f))
    return ts


def alternated(arms, n=5, before=None, clock=time.perf_counter):
    """{arm: call} -> {arm: [seconds of each call]}: n rounds of one call per arm, before() ahead of each outside the clock.  No warm-up: the caller's."""
    ts = {k: [] for k in arms}
    for _ in range(n):
        for k, f in arms.items():
            if before:
                before()
            t0 = clock()
            f()
            ts[k].append(clock() - t0)
    return ts


def interleaved(arms, reps, rounds, before=None, clock=time.perf_counter):
    """{arm: call} -> {arm: [the median of each repetition]}: a repetition is alternated() over `rounds` rounds."""
    meds = {k: [] for k in arms}
    for _ in range(reps):
        for k, ts in alternated(arms, rounds, before, clock).items():
            meds[k].append(statistics.median(ts))
    return meds


def pipelined(ctxs, nb, submit, consume, clock=time.perf_counter):
    """nb batches over the Q contexts, batch i on context i mod Q: batch j is synced -- and consume(ctx, slot, j) called, unless it is None -- when
    batch j + Q - 2 has been submitted with submit(ctx, slot, i), so Q - 1 chains are in flight with the consumers of the other contexts behind them.
    A context's sync_lines() ahead of its next batch waits for the consumer of its last one.  -> seconds, sum of sync(), sum of sync_lines()."""
    q = len(ctxs)
    lag = q - 2
    synced = lines = 0
    t0 = clock()
    for i in range(nb + lag):
        if i < nb:
            k = i % q
            lines += ctxs[k].sync_lines()
            submit(ctxs[k], k, i)
        j = i - lag
        if j >= 0:
            k = j % q
            synced += ctxs[k].sync()
            if consume is not None:
                consume(ctxs[k], k, j)
    for c in ctxs:
        lines += c.sync_lines()
    return clock() - t0, synced, lines


# ---- set-up

def synthetic_tokenizer(n_records=None, seed=None):
    """-> (the synthetic dictionary, a Tokenizer of it with its feature tables set, the known and the unknown feature table)."""
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict() if n_records is None else synth.build_dict(n_records, seed=seed)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return sd, tok, known, unk


class Resident:
    """One batch of sentences resident in HBM -- the text with 16 zero bytes behind it, int64 offsets, a record buffer of `cap` rows, record offsets and
    status -- tokenized once on `ctx`: n sentences, `total` bytes, `count` records."""

    def __init__(self, ctx, sents):
        import numpy as np
        import torch

        from kanpyo_amd.tokenizer import pack_sentences

        utf8, offs = pack_sentences(sents)
        dev = torch.device("cuda", 0)
        self.ctx, self.n, self.total = ctx, len(offs) - 1, int(offs[-1])
        self.cap = self.total + self.n + 64
        self.text = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
        self.offsets = torch.from_numpy(offs.astype(np.int64)).to(dev)
        self.records = torch.empty((self.cap, 6), dtype=torch.int32, device=dev)
        self.record_offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self.status = torch.empty(self.n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.count = self.tokenize()

    def tokenize(self):
        self.ctx.tokenize(self.text.data_ptr(), self.offsets.data_ptr(), self.n, self.total, self.records.data_ptr(), self.cap, self.record_offsets.data_ptr(), self.status.data_ptr())
        return self.ctx.sync()

    def args(self):
        """What every consumer of the records takes first: text, offsets, n, records, record offsets."""
        return self.text.data_ptr(), self.offsets.data_ptr(), self.n, self.records.data_ptr(), self.record_offsets.data_ptr()


def pipeline_rates(tok, sents, batch, q, consumers, reps):
    """The corpus cut into batches resident in HBM, q contexts with a record buffer and a 32 MiB output buffer each, and pipelined() over them once
    per consumer as a warm-up, then in `reps` rounds of one run each.  {name: consume or None} -> {name: [sentences/s of each run]}, {name: (records,
    what sync_lines reported) of its last run}.  consume(ctx, args, out, out_offsets) enqueues what reads a batch's records: args are what
    Resident.args() gives for a batch, out the slot's output buffer."""
    import numpy as np
    import torch

    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    dev = torch.device("cuda", 0)
    batches = []
    for lo in range(0, len(sents), batch):
        u, o = pack_sentences(sents[lo : lo + batch])
        batches.append((torch.from_numpy(u.copy()).to(dev), torch.from_numpy(o.astype(np.int64)).to(dev), len(o) - 1, int(o[-1]), int(o[-1]) + len(o)))
    ctxs = [DeviceContext(tok) for _ in range(q)]
    cap = max(b[4] for b in batches)
    bufs = [(torch.empty((cap, 6), dtype=torch.int32, device=dev), torch.empty(batch + 1, dtype=torch.int64, device=dev), torch.empty(batch, dtype=torch.uint8, device=dev),
             torch.empty(32 << 20, dtype=torch.uint8, device=dev), torch.empty(batch + 1, dtype=torch.int64, device=dev)) for _ in range(q)]

    def submit(c, k, i):
        (du, do, n, total, bcap), (dt, dto, dst, _, _) = batches[i], bufs[k]
        c.tokenize(du.data_ptr(), do.data_ptr(), n, total, dt.data_ptr(), bcap, dto.data_ptr(), dst.data_ptr())

    def run(name):
        f = consumers[name]

        def consume(c, k, j):
            (du, do, n, _, _), (dt, dto, _, out, out_off) = batches[j], bufs[k]
            f(c, (du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr()), out, out_off)

        seconds, records, reported = pipelined(ctxs, len(batches), submit, consume if f else None)
        counts[name] = (records, reported)
        return len(sents) / seconds

    res, counts = {name: [] for name in consumers}, {}
    for name in consumers:
        run(name)
    for _ in range(reps):
        for name in consumers:
            res[name].append(run(name))
    for c in ctxs:
        c.close()
    return res, counts


HALF = "ｱｲｳｴｵｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾅﾆﾇﾈﾉ"
FULL = "ＡＢＣＤＥＦＧＨＩＪ０１２３４５６７８９"


def dirty(s, rng):
    """Every tenth character, on average, becomes a half-width kana or a full-width letter or digit."""
    pool = HALF + FULL
    return "".join(pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.1 else c for c in s)
