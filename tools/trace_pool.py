#!/usr/bin/env python
"""Per-dispatch view of k_tokenize_pool in a rocprofv3 --kernel-trace CSV: durations grouped by grid size; with a second argument N also the LAST N
full-batch dispatches of the product kernel on their own -- the timed region of `bench.py --steps K` is its last 24 K full batches (what comes before is the
prewarm and the warmup, which run without the HIP events the timed region's launches are bracketed by): the figure bench.py's avg_kernel_ms is to be held against.
With N it also prints, per hardware queue (the trace's Queue_Id) and over that timed region (from the start of the N-th last full-batch dispatch to the
first 200 us in which no queue runs a kernel -- the host has left the loop that keeps eight batches in flight -- or the trace's end): the share of the time a kernel of the queue was running, the gaps between consecutive kernels of a batch (the pool launch, then the scan and
the compaction or the one launch that does both) and from a batch's last kernel to the next batch's pool launch, and the averages of the kernels behind
the pool launch -- the stream-side figures that the chip-side durations above do not show.
usage: python tools/trace_pool.py <kernel_trace.csv> [N]"""
import csv, sys
from collections import defaultdict
g = defaultdict(list)
full = []   # (start, duration) of the product kernel over full 4096-sentence batches (grid 1024 x 256 threads)
AUX = ("k_scan_counts_wave", "k_scan_counts", "k_compact8", "k_compact", "k_scan_compact", "k_aux_one_launch")   # (a name before its prefixes)
queues = defaultdict(list)   # Queue_Id -> (start, end, short kernel name) of the tokenize kernels and the kernels behind them
for r in csv.DictReader(open(sys.argv[1])):
    short = next((k for k in ("k_tokenize_pool", "k_tokenize_window", "k_tokenize_general") + AUX if "kgpu::" + k + "(" in r["Kernel_Name"] or "kgpu::" + k + "<" in r["Kernel_Name"]), None)
    if short:
        queues[r.get("Queue_Id", "?")].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    if "k_tokenize_pool" not in r["Kernel_Name"]:
        continue
    key = (r["Kernel_Name"].split("(")[0][-22:], r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")))
    dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    g[key].append(dur)
    if "pool<false" in r["Kernel_Name"] and key[1] == "262144":
        full.append((int(r["Start_Timestamp"]), dur))
def line(v):
    v = sorted(v)
    return f"n={len(v)} avg {sum(v)/len(v):.1f} us p10 {v[len(v)//10]:.1f} p50 {v[len(v)//2]:.1f} p90 {v[len(v)*9//10]:.1f} max {v[-1]:.1f}"
for k, v in sorted(g.items(), key=lambda kv: -len(kv[1])):
    print(f"{k}: {line(v)}")
if len(sys.argv) > 2 and full:
    n = int(sys.argv[2])
    full.sort()
    print(f"the last {min(n, len(full))} full-batch dispatches of the product kernel (the timed region): {line([d for _, d in full[-n:]])}")


def avg(v):
    return f"{sum(v) / len(v):.1f} us (n={len(v)})" if v else "-"


if len(sys.argv) > 2 and full:
    t0 = full[-min(n, len(full))][0]
    # the region ends where no queue runs a kernel for IDLE_NS: the host has left the loop that keeps eight batches in flight (what bench.py --full runs behind
    # it -- one context, which now visits every shared stream -- would otherwise stretch every queue's span)
    IDLE_NS = 200_000
    t1, busy_until = None, None
    for b, e, _ in sorted(k for ks in queues.values() for k in ks if k[0] >= t0):
        if busy_until is not None and b - busy_until >= IDLE_NS:
            t1 = busy_until
            break
        busy_until = e if busy_until is None else max(busy_until, e)
    t1 = busy_until if t1 is None else t1
    print(f"per hardware queue over the timed region ({len(queues)} queues; {(t1 - t0) / 1e6:.2f} ms, to the first {IDLE_NS // 1000} us without a kernel on any queue):")
    every = defaultdict(list)
    for q, ks in sorted(queues.items()):
        ks = sorted(k for k in ks if t0 <= k[0] < t1)
        if len(ks) < 2:
            continue
        span = (ks[-1][1] - ks[0][0]) / 1e3
        busy = sum(e - b for b, e, _ in ks) / 1e3
        inside, between, dur = defaultdict(list), [], defaultdict(list)
        for (b0, e0, k0), (b1, e1, k1) in zip(ks, ks[1:]):
            gap = (b1 - e0) / 1e3
            if k1 == "k_tokenize_pool":
                between.append(gap)   # the batch is over: the done event, the host, the next batch's launch
            else:
                inside[f"{k0[2:]} -> {k1[2:]}"].append(gap)
        for b, e, k in ks:
            dur[k].append((e - b) / 1e3)
            every[k].append((e - b) / 1e3)
        batches = len(dur["k_tokenize_pool"])
        print(f"  queue {q}: {len(ks)} kernels, {batches} pool launches over {span / 1e3:.2f} ms, {span / max(batches, 1):.1f} us a batch; a kernel runs {100 * busy / span:.1f} % of the time")
        for name, v in sorted(inside.items()):
            print(f"    gap {name}: avg {avg(v)}")
        print(f"    gap last kernel of a batch -> next pool launch: avg {avg(between)}")
        print("    " + ", ".join(f"{k} avg {avg(v)}" for k, v in sorted(dur.items())))
    print("  all queues: " + ", ".join(f"{k} avg {avg(v)} min {min(v):.1f} max {max(v):.1f}" for k, v in sorted(every.items())))
