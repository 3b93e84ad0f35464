#!/usr/bin/env python
"""The `kanpyo tokenize` output's rates (kgpu_format.hip and the lines entry points) on cfg 2: 100k sentences, batches of 4096, 8 contexts,
the synthetic 392k dictionary with synth.feature_tables.

    python tools/lines_rate.py [--out profiles/experiments/lines_rate.txt]

Legs: device-resident records alone vs records + render (alternated in one process); the render kernels under rocprofv3 --kernel-trace
--stats (a child process running the device leg alone) with bytes per token and bytes/s; kgpu_tokenize_batch_lines end to end (host
memory in, text out); the CLI on a file of the same sentences; dictfile.format_tokens on 2000 sentences for scale.

    python tools/lines_rate.py --split [--out profiles/experiments/split_device.txt]

The input side instead (kgpu_split.hip): the device split alone on a 64 MiB and a 4 MiB block resident in HBM (HIP events around enqueue -> sync,
and the k_split_* kernels under rocprofv3 in child processes) against the host kgpu_split_lines on the same blocks, alternated; then
kgpu_tokenize_text_lines against split_lines + tokenize_lines_packed and the CLI's --split device against --split host on the 100k-sentence file."""
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
HBM_TBS, PCIE_GBS = 6.3, 63.0


def setup():
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    sents = synth.make_corpus(sd, N, 1, "cfg2")
    return sd, tok, known, unk, sents, pack_sentences


def device_leg(tok, sents, pack_sentences, reps=3):
    import torch

    from kanpyo_amd.device import DeviceContext

    dev = torch.device("cuda", 0)
    batches = []
    for lo in range(0, len(sents), BATCH):
        u, o = pack_sentences(sents[lo : lo + BATCH])
        n, cap = len(o) - 1, int(o[-1]) + len(o)
        batches.append((torch.from_numpy(u.copy()).to(dev), torch.from_numpy(o.astype(np.int64)).to(dev), n, int(o[-1]), cap))
    ctxs = [DeviceContext(tok) for _ in range(Q)]
    bufs = []
    for _ in range(Q):
        cap = max(b[4] for b in batches)
        bufs.append((torch.empty((cap, 6), dtype=torch.int32, device=dev), torch.empty(BATCH + 1, dtype=torch.int64, device=dev),
                     torch.empty(BATCH, dtype=torch.uint8, device=dev), torch.empty(32 << 20, dtype=torch.uint8, device=dev),
                     torch.empty(BATCH + 1, dtype=torch.int64, device=dev)))
    stats = {"tokens": 0, "text": 0}
    LAG = Q - 2   # batch j is synced (and its render enqueued) when batch j + LAG is submitted: LAG + 1 chains in flight, the renders of the other contexts behind them

    def run(render):
        """Both legs run this same loop; only the render differs.  A render needs its own context's batch synced (kgpu_format_lines_device), not the others'."""
        nb = len(batches)
        t0 = time.perf_counter()
        for i in range(nb + LAG):
            if i < nb:
                k = i % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                stats["text"] += c.sync_lines()   # batch i - Q's render (a no-op in the records leg)
                du, do, n, total, cap = batches[i]
                c.tokenize(du.data_ptr(), do.data_ptr(), n, total, dt.data_ptr(), cap, dto.data_ptr(), dst.data_ptr())
            j = i - LAG
            if j >= 0:
                k = j % Q
                c, (dt, dto, dst, dtext, dtexto) = ctxs[k], bufs[k]
                stats["tokens"] += c.sync()
                if render:
                    du, do, n, total, cap = batches[j]
                    c.format_lines(du.data_ptr(), do.data_ptr(), n, dt.data_ptr(), dto.data_ptr(), dtext.data_ptr(), dtext.numel(), dtexto.data_ptr())
        for c in ctxs:
            stats["text"] += c.sync_lines()
        return len(sents) / (time.perf_counter() - t0)

    run(False), run(True)
    out = {"records": [], "render": []}
    for _ in range(reps):
        out["records"].append(run(False))
        stats["tokens"] = stats["text"] = 0
        out["render"].append(run(True))   # (the counts kept are the last render run's)
    for c in ctxs:
        c.close()
    return out, stats


WHITE_SPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(map(chr, range(0x2000, 0x200B))) + "\u2028\u2029\u202f\u205f\u3000"


def expected_stdout(sd, known, unk, lines) -> bytes:
    """What the reference CLI prints for these input lines, from the CPU oracle's tokens and the Python feature tables (not the library)."""
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    utf8, offs = pack_sentences([ln.rstrip(WHITE_SPACE) for ln in lines])
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 16)
    feats = ({}, {})
    out = []
    for i in range(len(offs) - 1):
        raw = utf8[int(offs[i]) : int(offs[i + 1])].tobytes()
        for t in exp.tokens[int(exp.offsets[i]) : int(exp.offsets[i + 1])]:
            cls, tid, pos, bl = int(t["cls"]), int(t["id"]), int(t["position"]), int(t["byte_len"])
            f = b""
            if cls != 0 and tid != 0:
                if tid not in feats[cls - 1]:
                    feats[cls - 1][tid] = ",".join((known if cls == 1 else unk).features(tid)).encode()
                f = feats[cls - 1][tid]
            out.append((b"EOS" if cls == 0 else raw[pos : pos + bl]) + b"\t" + f + b"\n")
    return b"".join(out)


def trace_leg(tmp):
    """rocprofv3 --kernel-trace --stats of a child running the device leg alone -> {kernel: (calls, total ns)}."""
    env = dict(os.environ)
    cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
           sys.executable, os.path.abspath(__file__), "--device-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tmp)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
    path = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def host_leg(tok, utf8, offs, say):
    """kgpu_tokenize_batch_lines end to end: host memory in, text out (caller-owned arrays, reused)."""
    first, _, _ = tok.tokenize_lines_packed(utf8, offs)
    out = (np.empty(first.size, dtype=np.uint8), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
    tok.tokenize_lines_packed(utf8, offs, out=out)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        t, _, _ = tok.tokenize_lines_packed(utf8, offs, out=out)
        ts.append(time.perf_counter() - t0)
    dt = float(np.median(ts))
    say(f"kgpu_tokenize_batch_lines, host in / text out: {N / dt / 1e6:.2f} M sentences/s, {t.size / dt / 1e9:.1f} GB/s of text "
        f"({t.size / dt / 1e9 / PCIE_GBS * 100:.0f} % of PCIe Gen5 x16's {PCIE_GBS:.0f} GB/s; target 20 GB/s); median of {len(ts)}: "
        + ", ".join(f"{t.size / x / 1e9:.1f}" for x in ts) + " GB/s")


COPY_TBS = 6.29   # MI355X device-to-device copy rate


def split_blocks(sd):
    """The 64 MiB block of tests/test_gpu_split.py (cfg 2 sentences joined with "\n", "\r\n" and U+3000 "\n") and its first 4 MiB cut behind a newline."""
    from kanpyo_amd import synth

    sents = synth.make_corpus(sd, (64 << 20) // 112 + 20000, 21, "cfg2")
    tails = ["\n", "\r\n", "\u3000\n"]
    big = np.frombuffer("".join(s + tails[i % 3] for i, s in enumerate(sents)).encode(), dtype=np.uint8)[: 64 << 20]
    cut = int(np.flatnonzero(big[: 4 << 20] == 10)[-1]) + 1
    return {"64 MiB": big, "4 MiB": big[:cut]}


class DeviceSplit:
    """One block resident in HBM and the buffers of its split, on a context that runs on a torch stream (so that torch's events bracket its work)."""

    def __init__(self, tok, block):
        import torch

        from kanpyo_amd.device import DeviceContext

        dev = torch.device("cuda", 0)
        self.torch, self.n = torch, int(block.size)
        self.stream = torch.cuda.Stream(device=dev)
        self.ctx = DeviceContext(tok, self.stream.cuda_stream)
        self.cap = int(np.count_nonzero(block == 10)) + 2
        self.d_in = torch.from_numpy(block.copy()).to(dev)
        self.d_out = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.d_off = torch.empty(self.cap, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def once(self):
        self.ctx.split_lines(self.d_in.data_ptr(), self.n, self.d_out.data_ptr(), self.d_off.data_ptr(), self.cap)
        return self.ctx.sync_split()

    def timed(self, reps):
        """-> seconds per enqueue -> sync, from HIP events on the context's stream around `reps` of them."""
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for _ in range(reps):
            self.once()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps


def host_split_timed(block, reps):
    """-> seconds per kgpu_split_lines call (the C function alone, buffers allocated and touched beforehand)."""
    import ctypes as C

    from kanpyo_amd import _lib

    L = _lib.lib()
    out = np.zeros(block.size, dtype=np.uint8)
    offs = np.zeros(int(np.count_nonzero(block == 10)) + 2, dtype=np.uint64)
    n = C.c_uint64(0)
    t0 = time.perf_counter()
    for _ in range(reps):
        _lib.check(L.kgpu_split_lines(block.ctypes.data, block.size, out.ctypes.data, offs.ctypes.data, offs.size, C.byref(n)))
    return (time.perf_counter() - t0) / reps, int(n.value), int(offs[int(n.value)])


def split_child(path, reps):
    """The child of the rocprofv3 run: `reps` device splits of the block in the file, on a small dictionary (the split needs none of it)."""
    import torch  # noqa: F401

    from kanpyo_amd import Tokenizer, synth

    ds = DeviceSplit(Tokenizer(synth.build_dict(20000, seed=11).dict), np.load(path))
    for _ in range(reps):
        ds.once()


def split_trace(tmp, path, reps):
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
           sys.executable, os.path.abspath(__file__), "--split-child", path, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
    out = {}
    with open(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]) as f:
        for row in csv.DictReader(f):
            if "k_split_" in row["Name"]:
                out[row["Name"].split("(")[0].split("::")[-1]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def spread(xs, scale=1.0, unit="s"):
    return f"median {np.median(xs) * scale:.3f} {unit} (runs: {', '.join(f'{x * scale:.3f}' for x in xs)})"


def split_main(args, say):
    sd, tok, known, unk, sents, pack_sentences = setup()
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import split_lines

    say(f"# tools/lines_rate.py --split: read_line + trim_end on the device (kgpu_split.hip) against the host kgpu_split_lines; library {_lib.kernel_source_hash()}")
    ok = True
    blocks = split_blocks(sd)
    for name, block in blocks.items():
        ds = DeviceSplit(tok, block)
        n_lines, n_bytes = ds.once()
        h_dt, h_lines, h_bytes = host_split_timed(block, 1)   # warm-up pass of both, and the same counts
        assert (n_lines, n_bytes) == (h_lines, h_bytes), ((n_lines, n_bytes), (h_lines, h_bytes))
        reps_d = max(3, int(0.25 / max(ds.timed(3), 1e-6)))
        reps_h = max(1, int(0.25 / h_dt))
        dev_t, host_t = [], []
        for _ in range(5):   # alternated in one process
            dev_t.append(ds.timed(reps_d))
            host_t.append(host_split_timed(block, reps_h)[0])
        d, h = min(dev_t), min(host_t)
        moved = 2 * block.size + n_bytes + (n_lines + 1) * 8
        say(f"{name} block: {block.size} bytes, {n_lines} lines, {n_bytes} bytes kept")
        say(f"  device, input resident, HIP events around enqueue -> sync, {reps_d} per window: best of 5 {d * 1e6:.1f} us = {block.size / d / 1e9:.1f} GB/s of input"
            f"  (windows: {', '.join(f'{x * 1e6:.1f}' for x in dev_t)} us)")
        say(f"  host kgpu_split_lines, {reps_h} per window: best of 5 {h * 1e3:.2f} ms = {block.size / h / 1e9:.2f} GB/s of input"
            f"  (windows: {', '.join(f'{x * 1e3:.2f}' for x in host_t)} ms)")
        ratio = h / d
        line = f"  device / host: {ratio:.1f} x"
        if name == "64 MiB":
            ok = ratio >= 10
            line += f"  (acceptance: >= 10 x on this block: {'met' if ok else 'NOT MET'})"
        say(line)
        if not args.no_trace:
            reps = 20 if name == "64 MiB" else 200
            with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
                path = os.path.join(tmp, "block.npy")
                np.save(path, block)
                ks = split_trace(tmp, path, reps)
            total = sum(ns for _, ns in ks.values())
            for k in sorted(ks):
                c, ns = ks[k]
                say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
            per = total / reps
            say(f"  kernels (rocprofv3 --kernel-trace --stats, a run of its own): {per / 1e3:.1f} us per split; bytes moved (input read by two passes, kept bytes and offsets "
                f"written) {moved / 1e6:.1f} MB -> {moved / per:.0f} GB/s = {moved / per / (COPY_TBS * 1e3) * 100:.1f} % of the {COPY_TBS} TB/s copy rate")
        ds.ctx.close()

    # end to end on the 100k-sentence file of the CLI leg
    data = "\n".join(s.replace("\n", " ") for s in sents).encode() + b"\n"
    block = np.frombuffer(data, dtype=np.uint8)
    want = tok.tokenize_lines_packed(*split_lines(block))
    got = tok.tokenize_text_lines(block)
    same = all(np.array_equal(a, b) for a, b in zip(got, want))
    t_new, t_old, t_split = [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        tok.tokenize_text_lines(block)
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        u, o = split_lines(block)
        t1 = time.perf_counter()
        tok.tokenize_lines_packed(u, o)
        t_old.append(time.perf_counter() - t0)
        t_split.append(t1 - t0)
    say(f"end to end, {N} cfg 2 lines ({block.size / 1e6:.1f} MB in, {want[0].size / 1e6:.0f} MB of text out), outputs identical: {same}")
    say(f"  tokenize_text_lines (device split):                   {spread(t_new, 1e3, 'ms')}")
    say(f"  split_lines + tokenize_lines_packed (host split):     {spread(t_old, 1e3, 'ms')}")
    say(f"    of which split_lines (the wrapper's count pass + kgpu_split_lines): {spread(t_split, 1e3, 'ms')} = {np.median(t_split) / np.median(t_old) * 100:.0f} % of that path's wall time")
    say(f"  -> {'the device split' if np.median(t_new) < np.median(t_old) else 'the host split + chunk pipeline'} is faster, {max(np.median(t_new), np.median(t_old)) / min(np.median(t_new), np.median(t_old)):.2f} x")
    from kanpyo_amd.dictfile import DictFile, save_dict

    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        dpath, ipath = os.path.join(tmp, "t.dict"), os.path.join(tmp, "in.txt")
        save_dict(DictFile(sd.dict, known, unk), dpath)
        with open(ipath, "wb") as f:
            f.write(data)
        wall, outs = {"host": [], "device": []}, {}
        for _ in range(3):
            for mode in ("host", "device"):
                with open(ipath, "rb") as fi:
                    t0 = time.perf_counter()
                    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", dpath, "--split", mode], stdin=fi,
                                       stdout=subprocess.PIPE, cwd=ROOT)
                    wall[mode].append(time.perf_counter() - t0)
                if r.returncode != 0:
                    raise RuntimeError(f"CLI --split {mode} exited {r.returncode}")
                outs[mode] = r.stdout
        say(f"python -m kanpyo_amd tokenize < {N} lines (process start, dictionary load and upload included), stdout identical: {outs['host'] == outs['device']}")
        say(f"  --split host:   {spread(wall['host'])}")
        say(f"  --split device: {spread(wall['device'])}")
        say(f"  -> {'--split device' if np.median(wall['device']) < np.median(wall['host']) else '--split host'} is faster, by {abs(np.median(wall['device']) - np.median(wall['host'])):.3f} s")
    return ok and same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", action="store_true", help="the input side: the device split against the host splitter")
    ap.add_argument("--split-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--host-only", action="store_true", help="the kgpu_tokenize_batch_lines leg alone (A/B of builds through KGPU_LIB)")
    args = ap.parse_args()
    if args.split_child:
        split_child(args.split_child, args.reps)
        return
    if args.split:
        lines = []
        ok = split_main(args, lambda s: (print(s, flush=True), lines.append(s)))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(0 if ok else 1)
    sd, tok, known, unk, sents, pack_sentences = setup()
    if args.device_only:
        device_leg(tok, sents, pack_sentences, reps=1)
        return
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731
    utf8, offs = pack_sentences(sents)
    say(f"# tools/lines_rate.py: cfg 2, {N} sentences ({int(offs[-1]) / N:.0f} bytes each), batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables")

    if args.host_only:
        host_leg(tok, utf8, offs, say)
        return
    dev, st = device_leg(tok, sents, pack_sentences)
    rec, ren = np.median(dev["records"]), np.median(dev["render"])
    tokens, text = st["tokens"], st["text"]
    say(f"device-resident, records alone:    {rec / 1e6:.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in dev['records'])})")
    say(f"device-resident, records + render: {ren / 1e6:.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in dev['render'])}) = {ren / rec:.2f} x records alone (target >= 0.85)")
    say(f"  {tokens} tokens, {text} bytes of text: {tokens / N:.1f} tokens and {text / N:.0f} bytes per sentence, {text / tokens:.1f} bytes per token")

    if not args.no_trace:
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            ks = trace_leg(tmp)
        names = [k for k in ks if "k_lines_" in k]
        total_ns = sum(ks[k][1] for k in names)
        for k in sorted(names):
            c, ns = ks[k]
            say(f"  {k.split('(')[0]:<28} {c} calls, {ns / 1e3 / c:8.1f} us per call, {ns / 1e6:8.2f} ms in all")
        feat = text - tokens * 2 - int(offs[-1]) - 3 * N   # text = surfaces (input bytes + "EOS") + tab + newline + features
        moved = tokens * 24 * 2 + int(offs[-1]) + feat + text + N * 32
        say(f"  render kernels: {total_ns / 1e6:.2f} ms for {N} sentences; bytes moved (records read twice, surfaces, features, text written, offsets) "
            f"{moved / 1e6:.0f} MB = {moved / tokens:.0f} B/token -> {moved / total_ns:.0f} GB/s, {moved / total_ns / (HBM_TBS * 1e3) * 100:.1f} % of {HBM_TBS} TB/s")
        other = sum(ns for k, (c, ns) in ks.items() if k not in names)
        calls = ks[names[0]][0] if names else 1
        say(f"  (the same trace: tokenize chain + scan/compaction {other / 1e6:.2f} ms over twice as many batches: "
            f"{other / 2e3 / calls:.1f} us of kernel time per 4096-sentence batch, render {total_ns / 1e3 / calls:.1f} us: "
            f"records + render can reach at most {other / 2 / (other / 2 + total_ns):.2f} x records alone where kernel time is the bound)")

    host_leg(tok, utf8, offs, say)

    # the CLI on a file of the same sentences
    from kanpyo_amd.dictfile import DictFile, save_dict

    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        dpath, ipath = os.path.join(tmp, "t.dict"), os.path.join(tmp, "in.txt")
        save_dict(DictFile(sd.dict, known, unk), dpath)
        with open(ipath, "wb") as f:
            f.write("\n".join(s.replace("\n", " ") for s in sents).encode() + b"\n")
        with open(ipath, "rb") as fi:
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", dpath], stdin=fi, stdout=subprocess.PIPE, cwd=ROOT, timeout=600)
            dt = time.perf_counter() - t0
        want = expected_stdout(sd, known, unk, [s.replace("\n", " ") for s in sents])
        say(f"python -m kanpyo_amd tokenize < {N} lines: {dt:.2f} s wall (process start, dictionary load and upload included), "
            f"{len(r.stdout) / 1e6:.0f} MB of stdout, exit {r.returncode}; byte-identical to the expected bytes (oracle tokens + "
            f"MorphFeatureTable.features, lines trimmed as trim_end does): {r.stdout == want}")

    # format_tokens, for scale
    from kanpyo_amd.dictfile import format_tokens

    df = DictFile(sd.dict, known, unk)
    toks = tok.tokenize_batch(sents[:2000])
    t0 = time.perf_counter()
    for row in toks:
        format_tokens(row, df)
    dt = time.perf_counter() - t0
    say(f"dictfile.format_tokens (Python loop over Token objects), 2000 sentences: {2000 / dt / 1e3:.1f} k sentences/s")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
