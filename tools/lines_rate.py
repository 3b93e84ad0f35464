#!/usr/bin/env python
"""The `kanpyo tokenize` output's rates (kgpu_format.hip and the lines entry points) on cfg 2: 100k sentences, batches of 4096, 8 contexts,
the synthetic 392k dictionary with synth.feature_tables.

    python tools/lines_rate.py [--out profiles/experiments/lines_rate.txt] [--no-trace] [--host-only]

Legs, run by tools/measure.py (each a process of its own under a time limit; trouble in one ends the run):
  device   device-resident records alone against records + render through measure.pipeline_rates() (measure.pipelined() with the render as the consumer).
  trace    measure.trace() over `--device-only` (the pipeline once per arm): the render kernels, bytes per token and bytes/s.
  host     kgpu_tokenize_batch_lines end to end, host memory in, text out (--host-only: this leg alone, for an A/B of builds through KGPU_LIB).
  cli      the CLI on a file of the same sentences against the bytes the CPU oracle and the feature tables give; dictfile.format_tokens on 2000
           sentences for scale.

    python tools/lines_rate.py --split [--out profiles/experiments/split_device.txt] [--no-trace]

The input side instead (kgpu_split.hip).  Legs: per block (64 MiB and 4 MiB resident in HBM) the device split alone, HIP events around enqueue -> sync,
against the host kgpu_split_lines on the same block, alternated, then the k_split_* kernels through measure.trace(); kgpu_tokenize_text_lines against
split_lines + tokenize_lines_packed; the CLI's --split device against --split host on the 100k-sentence file."""
import os
import sys
import tempfile
import time

import numpy as np

import measure

N, BATCH, Q = 100_000, 4096, 8
HBM_TBS, PCIE_GBS = 6.3, 63.0
COPY_TBS = 6.29   # MI355X device-to-device copy rate
ARGS = None       # the command line's


def setup():
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, known, unk = measure.synthetic_tokenizer()
    sents = synth.make_corpus(sd, N, 1, "cfg2")
    return sd, tok, known, unk, sents, pack_sentences


def header(sents_bytes):
    return f"# tools/lines_rate.py: cfg 2, {N} sentences ({sents_bytes / N:.0f} bytes each), batches of {BATCH}, {Q} contexts; synthetic 392k dictionary + synth.feature_tables"


def device_runs(tok, sents, reps):
    """-> {"records": [sentences/s], "render": [...]}, {arm: (tokens, bytes of text) of its last run}."""
    render = lambda c, args, out, out_off: c.format_lines(*args, out.data_ptr(), out.numel(), out_off.data_ptr())   # noqa: E731
    return measure.pipeline_rates(tok, sents, BATCH, Q, {"records": None, "render": render}, reps)


def device_only():
    """The program of the trace leg."""
    sd, tok, known, unk, sents, pack_sentences = setup()
    _, counts = device_runs(tok, sents, reps=1)
    print(f"COUNTS {counts['render'][0]} {counts['render'][1]} {int(pack_sentences(sents)[1][-1])}", flush=True)


def leg_device(say):
    sd, tok, known, unk, sents, pack_sentences = setup()
    say(header(int(pack_sentences(sents)[1][-1])))
    dev, counts = device_runs(tok, sents, reps=3)
    rec, ren = measure.summary(dev["records"])[0], measure.summary(dev["render"])[0]
    tokens, text = counts["render"]
    say(f"device-resident, records alone:    {rec / 1e6:.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in dev['records'])})")
    say(f"device-resident, records + render: {ren / 1e6:.1f} M sentences/s  (runs: {', '.join(f'{x / 1e6:.1f}' for x in dev['render'])}) = {ren / rec:.2f} x records alone (target >= 0.85)")
    say(f"  {tokens} tokens, {text} bytes of text: {tokens / N:.1f} tokens and {text / N:.0f} bytes per sentence, {text / tokens:.1f} bytes per token")
    return True


def leg_trace(say):
    stdout, ks = measure.trace(__file__, ["--device-only"], 400)
    tokens, text, in_bytes = (int(x) for x in [ln for ln in stdout.splitlines() if ln.startswith("COUNTS ")][-1].split()[1:])
    names = [k for k in ks if k.startswith("k_lines_")]
    total_ns = sum(ks[k][1] for k in names)
    for k in sorted(names):
        c, ns = ks[k]
        say(f"  {k:<28} {c} calls, {ns / 1e3 / c:8.1f} us per call, {ns / 1e6:8.2f} ms in all")
    feat = text - tokens * 2 - in_bytes - 3 * N   # text = surfaces (input bytes + "EOS") + tab + newline + features
    moved = tokens * 24 * 2 + in_bytes + feat + text + N * 32
    say(f"  render kernels: {total_ns / 1e6:.2f} ms for {N} sentences; bytes moved (records read twice, surfaces, features, text written, offsets) "
        f"{moved / 1e6:.0f} MB = {moved / tokens:.0f} B/token -> {moved / total_ns:.0f} GB/s, {moved / total_ns / (HBM_TBS * 1e3) * 100:.1f} % of {HBM_TBS} TB/s")
    other = sum(ns for k, (c, ns) in ks.items() if k not in names)
    calls = ks[names[0]][0] if names else 1
    say(f"  (the same trace: tokenize chain + scan/compaction {other / 1e6:.2f} ms over twice as many batches: "
        f"{other / 2e3 / calls:.1f} us of kernel time per 4096-sentence batch, render {total_ns / 1e3 / calls:.1f} us: "
        f"records + render can reach at most {other / 2 / (other / 2 + total_ns):.2f} x records alone where kernel time is the bound)")
    return True


def leg_host(say):
    """kgpu_tokenize_batch_lines end to end: host memory in, text out (caller-owned arrays, reused)."""
    sd, tok, known, unk, sents, pack_sentences = setup()
    utf8, offs = pack_sentences(sents)
    if ARGS.host_only:
        say(header(int(offs[-1])))
    first, _, _ = tok.tokenize_lines_packed(utf8, offs)
    out = (np.empty(first.size, dtype=np.uint8), np.empty(N + 1, dtype=np.uint64), np.empty(N, dtype=np.uint8))
    tok.tokenize_lines_packed(utf8, offs, out=out)
    ts = measure.alternated({"lines": lambda: tok.tokenize_lines_packed(utf8, offs, out=out)})["lines"]
    dt, size = measure.summary(ts)[0], first.size
    say(f"kgpu_tokenize_batch_lines, host in / text out: {N / dt / 1e6:.2f} M sentences/s, {size / dt / 1e9:.1f} GB/s of text "
        f"({size / dt / 1e9 / PCIE_GBS * 100:.0f} % of PCIe Gen5 x16's {PCIE_GBS:.0f} GB/s; target 20 GB/s); median of {len(ts)}: "
        + ", ".join(f"{size / x / 1e9:.1f}" for x in ts) + " GB/s")
    return True


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


def cli(dpath, ipath, *more):
    """One run of the CLI on the file, a step of its own (it takes a few seconds: a minute is its limit) -> seconds, stdout.  Any status but 0
    ends the leg, and with it the run."""
    with open(ipath, "rb") as fi:
        t0 = time.perf_counter()
        rc, stdout, err = measure.step([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", dpath, *more], 60, stdin=fi, text=False)
        dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"CLI {' '.join(more)} exited {rc}: {err.decode(errors='replace')}")
    return dt, stdout


def leg_cli(say):
    from kanpyo_amd.dictfile import DictFile, format_tokens, save_dict

    sd, tok, known, unk, sents, pack_sentences = setup()
    df = DictFile(sd.dict, known, unk)
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:   # the CLI on a file of the same sentences
        dpath, ipath = os.path.join(tmp, "t.dict"), os.path.join(tmp, "in.txt")
        save_dict(df, dpath)
        with open(ipath, "wb") as f:
            f.write("\n".join(s.replace("\n", " ") for s in sents).encode() + b"\n")
        dt, stdout = cli(dpath, ipath)
    want = expected_stdout(sd, known, unk, [s.replace("\n", " ") for s in sents])
    say(f"python -m kanpyo_amd tokenize < {N} lines: {dt:.2f} s wall (process start, dictionary load and upload included), "
        f"{len(stdout) / 1e6:.0f} MB of stdout, exit 0; byte-identical to the expected bytes (oracle tokens + "
        f"MorphFeatureTable.features, lines trimmed as trim_end does): {stdout == want}")
    toks = tok.tokenize_batch(sents[:2000])   # format_tokens, for scale
    t0 = time.perf_counter()
    for row in toks:
        format_tokens(row, df)
    dt = time.perf_counter() - t0
    say(f"dictfile.format_tokens (Python loop over Token objects), 2000 sentences: {2000 / dt / 1e3:.1f} k sentences/s")
    return True


# ---- --split

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
    """-> seconds per kgpu_split_lines call (the C function alone, buffers allocated and touched beforehand), lines, bytes kept."""
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
    """The program of the split's trace legs: `reps` device splits of the block in the file, on a small dictionary (the split needs none of it)."""
    ds = DeviceSplit(measure.synthetic_tokenizer(20000, seed=11)[1], np.load(path))
    for _ in range(reps):
        ds.once()


def spread(xs, scale=1.0, unit="s"):
    return f"median {measure.summary(xs)[0] * scale:.3f} {unit} (runs: {', '.join(f'{x * scale:.3f}' for x in xs)})"


def leg_split(say, name):
    sd, tok, _, _ = measure.synthetic_tokenizer()
    block = split_blocks(sd)[name]
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
    say(f"{name} block: {block.size} bytes, {n_lines} lines, {n_bytes} bytes kept")
    say(f"  device, input resident, HIP events around enqueue -> sync, {reps_d} per window: best of 5 {d * 1e6:.1f} us = {block.size / d / 1e9:.1f} GB/s of input"
        f"  (windows: {', '.join(f'{x * 1e6:.1f}' for x in dev_t)} us)")
    say(f"  host kgpu_split_lines, {reps_h} per window: best of 5 {h * 1e3:.2f} ms = {block.size / h / 1e9:.2f} GB/s of input"
        f"  (windows: {', '.join(f'{x * 1e3:.2f}' for x in host_t)} ms)")
    ratio, ok = h / d, True
    line = f"  device / host: {ratio:.1f} x"
    if name == "64 MiB":
        ok = ratio >= 10
        line += f"  (acceptance: >= 10 x on this block: {'met' if ok else 'NOT MET'})"
    say(line)
    ds.ctx.close()
    return ok


def leg_split_trace(say, name):
    from kanpyo_amd import synth

    block = split_blocks(synth.build_dict())[name]
    _, n_lines, n_bytes = host_split_timed(block, 1)   # (the host function's counts are the device's: the leg before this one has checked it)
    moved = 2 * block.size + n_bytes + (n_lines + 1) * 8
    reps = 20 if name == "64 MiB" else 200
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        path = os.path.join(tmp, "block.npy")
        np.save(path, block)
        _, ks = measure.trace(__file__, ["--split-child", path, "--reps", str(reps)], 300)
    ks = {k: v for k, v in ks.items() if k.startswith("k_split_")}
    total = sum(ns for _, ns in ks.values())
    for k in sorted(ks):
        c, ns = ks[k]
        say(f"  {k:<16} {c} calls, {ns / 1e3 / c:8.1f} us per call")
    per = total / reps
    say(f"  kernels (rocprofv3 --kernel-trace --stats, a run of its own): {per / 1e3:.1f} us per split; bytes moved (input read by two passes, kept bytes and offsets "
        f"written) {moved / 1e6:.1f} MB -> {moved / per:.0f} GB/s = {moved / per / (COPY_TBS * 1e3) * 100:.1f} % of the {COPY_TBS} TB/s copy rate")
    return True


def file_of(sents):
    return "\n".join(s.replace("\n", " ") for s in sents).encode() + b"\n"


def leg_split_end_to_end(say):
    """On the 100k-sentence file of the CLI leg."""
    from kanpyo_amd.tokenizer import split_lines

    sd, tok, known, unk, sents, pack_sentences = setup()
    block = np.frombuffer(file_of(sents), dtype=np.uint8)
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
    m_new, m_old, m_split = (measure.summary(x)[0] for x in (t_new, t_old, t_split))
    say(f"end to end, {N} cfg 2 lines ({block.size / 1e6:.1f} MB in, {want[0].size / 1e6:.0f} MB of text out), outputs identical: {same}")
    say(f"  tokenize_text_lines (device split):                   {spread(t_new, 1e3, 'ms')}")
    say(f"  split_lines + tokenize_lines_packed (host split):     {spread(t_old, 1e3, 'ms')}")
    say(f"    of which split_lines (the wrapper's count pass + kgpu_split_lines): {spread(t_split, 1e3, 'ms')} = {m_split / m_old * 100:.0f} % of that path's wall time")
    say(f"  -> {'the device split' if m_new < m_old else 'the host split + chunk pipeline'} is faster, {max(m_new, m_old) / min(m_new, m_old):.2f} x")
    return same


def leg_split_cli(say):
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile, save_dict

    sd = synth.build_dict()   # (no device in this leg's own process: the CLI runs are its steps)
    known, unk = synth.feature_tables(sd)
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        dpath, ipath = os.path.join(tmp, "t.dict"), os.path.join(tmp, "in.txt")
        save_dict(DictFile(sd.dict, known, unk), dpath)
        with open(ipath, "wb") as f:
            f.write(file_of(synth.make_corpus(sd, N, 1, "cfg2")))
        wall, outs = {"host": [], "device": []}, {}
        for _ in range(3):
            for mode in ("host", "device"):
                dt, outs[mode] = cli(dpath, ipath, "--split", mode)
                wall[mode].append(dt)
    m = {k: measure.summary(v)[0] for k, v in wall.items()}
    say(f"python -m kanpyo_amd tokenize < {N} lines (process start, dictionary load and upload included), stdout identical: {outs['host'] == outs['device']}")
    say(f"  --split host:   {spread(wall['host'])}")
    say(f"  --split device: {spread(wall['device'])}")
    say(f"  -> {'--split device' if m['device'] < m['host'] else '--split host'} is faster, by {abs(m['device'] - m['host']):.3f} s")
    return True


LEGS = {"device": (leg_device, 400), "trace": (leg_trace, 500), "host": (leg_host, 400), "cli": (leg_cli, 500)}
SPLIT_LEGS = {"64 MiB": (lambda say: leg_split(say, "64 MiB"), 400), "64 MiB trace": (lambda say: leg_split_trace(say, "64 MiB"), 400),
              "4 MiB": (lambda say: leg_split(say, "4 MiB"), 400), "4 MiB trace": (lambda say: leg_split_trace(say, "4 MiB"), 400),
              "end to end": (leg_split_end_to_end, 400), "cli": (leg_split_cli, 500)}   # (six CLI steps of 60 s at the most)


def main():
    global ARGS
    ap = measure.parser(__doc__, no_trace=True)
    ap.add_argument("--split", action="store_true", help="the input side: the device split against the host splitter")
    ap.add_argument("--split-child", default=None, help=measure.argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=1, help=measure.argparse.SUPPRESS)
    ap.add_argument("--device-only", action="store_true", help="the pipeline of the device leg once per arm, nothing printed but its counts: the trace leg's program")
    ap.add_argument("--host-only", action="store_true", help="the kgpu_tokenize_batch_lines leg alone (A/B of builds through KGPU_LIB)")
    ARGS = args = ap.parse_args()
    if args.split_child:
        split_child(args.split_child, args.reps)
    elif args.device_only:
        device_only()
    elif args.split:
        measure.main(__file__, args, SPLIT_LEGS, lambda: f"# tools/lines_rate.py --split: read_line + trim_end on the device (kgpu_split.hip) against the host kgpu_split_lines; library {measure.library_hash()}",
                     skip=[n for n in SPLIT_LEGS if args.no_trace and n.endswith("trace")], leg_args=["--split"])
    else:   # (no header of the parent's: the first leg says it, with the size of the corpus it has built)
        skip = [n for n in LEGS if n != "host"] if args.host_only else ["trace"] if args.no_trace else []
        measure.main(__file__, args, LEGS, None, skip=skip, leg_args=["--host-only"] if args.host_only else [])


if __name__ == "__main__":
    main()
