"""tools/measure.py, the harness of the measuring tools, on the CPU: the leg driver with a fake tool, the kernel-name cut and the trace readers on
crafted and on committed CSVs, the trace call with a stand-in profiler, the timing loops with a counting clock, the pipelined loop with fake
contexts, and `--help` of every ported tool (none of them may open a device, or build a dictionary, before it has parsed its command line)."""
import csv
import glob
import os
import stat
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

# measure.py sets KANPYO_SYNTH_CACHE's default and puts the repository on sys.path, as a tool's process needs; pytest imports this module at
# collection, so neither may stay behind for the other tests of the session (a cached synthetic dictionary from outside the repository)
_ENV, _PATH = os.environ.get("KANPYO_SYNTH_CACHE"), list(sys.path)
sys.path.insert(0, TOOLS)
import measure  # noqa: E402

sys.path[:] = _PATH
if _ENV is None:
    os.environ.pop("KANPYO_SYNTH_CACHE", None)

PORTED = ["count_timing", "decode_rate", "encode_rate", "pack_rate", "words_rate", "wordpiece_rate", "lines_rate", "graphviz_rate", "normalize_timing",
          "align_timing", "encode_spans_timing", "ablate"]


def test_import_leaves_the_session_as_it_was():
    assert os.environ.get("KANPYO_SYNTH_CACHE") == _ENV and TOOLS not in sys.path


def test_import_needs_no_torch():
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); import measure; assert 'torch' not in sys.modules", TOOLS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- 1. the leg driver

FAKE = """\
import os, signal, sys, time
sys.path.insert(0, {tools!r})
import measure

def mark(name):
    open(os.path.join({d!r}, name + ".ran"), "w").close()

def a(say):
    mark("a"); say("a one"); say("a two"); return True

def b(say):
    mark("b")
{b}

def c(say):
    mark("c"); say("c one"); return True

LEGS = {{"a": (a, 30), "b": (b, {limit}), "c": (c, 30)}}
args = measure.parser("fake").parse_args()
measure.main(__file__, args, LEGS, lambda: "# header")
"""
B = {
    "ok": "say('b one'); return True",
    "not met": "say('b NOT MET'); return False",
    "exit 1": "sys.stderr.write('b is in trouble\\n'); sys.exit(1)",
    "abort": "sys.stderr.write('b is in trouble\\n'); sys.stderr.flush(); os.abort()",
    "segv": "sys.stderr.write('b is in trouble\\n'); sys.stderr.flush(); os.kill(os.getpid(), signal.SIGSEGV); time.sleep(5)",
    "sleep": "sys.stderr.write('b is in trouble\\n'); sys.stderr.flush(); time.sleep(30)",
}


def run_fake(tmp_path, b):
    tool, out = tmp_path / "fake_tool.py", tmp_path / "out.txt"
    tool.write_text(FAKE.format(tools=TOOLS, d=str(tmp_path), b=textwrap.indent(B[b], "    "), limit=1 if b == "sleep" else 30))
    r = subprocess.run([sys.executable, str(tool), "--out", str(out)], capture_output=True, text=True)
    ran = {n for n in "abc" if (tmp_path / f"{n}.ran").exists()}
    return r, out.read_text().splitlines(), ran


def test_legs_not_met_goes_on_and_ends_with_1(tmp_path):
    r, lines, ran = run_fake(tmp_path, "not met")
    assert ran == {"a", "b", "c"} and r.returncode == 1
    assert lines == ["# header", "a one", "a two", "b NOT MET", "c one"] and r.stdout.splitlines() == lines


def test_legs_all_pass(tmp_path):
    r, lines, ran = run_fake(tmp_path, "ok")
    assert ran == {"a", "b", "c"} and r.returncode == 0 and lines == ["# header", "a one", "a two", "b one", "c one"]


@pytest.mark.parametrize("b, status", [("exit 1", 1), ("abort", -6), ("segv", -11), ("sleep", 124)])
def test_legs_trouble_ends_the_run(tmp_path, b, status):
    r, lines, ran = run_fake(tmp_path, b)
    assert ran == {"a", "b"}, "no leg is started behind one that ended badly"
    assert r.returncode == 1
    assert lines[:3] == ["# header", "a one", "a two"]
    assert lines[3].startswith(f"leg b ended with status {status}; its stderr ends: ") and lines[3] in r.stdout
    assert "b is in trouble" in "\n".join(lines[3:]) and "c one" not in lines


def test_legs_can_be_skipped_and_carry_facts(tmp_path):
    tool = tmp_path / "t.py"
    tool.write_text(textwrap.dedent(f"""\
        import sys
        sys.path.insert(0, {TOOLS!r})
        import measure
        def a(say): say("a"); measure.carry(x=1.5); return True
        def b(say): say("b"); return True
        def c(say): say(f"c got {{measure.carried()['x']}}"); return True
        args = measure.parser("fake").parse_args()
        measure.main(__file__, args, {{"a": (a, 30), "b": (b, 30), "c": (c, 30)}}, None, skip=["b"], headings=True)
        """))
    r = subprocess.run([sys.executable, str(tool), "--out", str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["a", "c got 1.5"]
    assert (tmp_path / "o").read_text().splitlines() == ["[a]", "a", "[c]", "c got 1.5"]


# ---- 2. names

STATS = sorted(glob.glob(os.path.join(ROOT, "profiles", "**", "*kernel_stats.csv"), recursive=True))


def test_kernel_names():
    f = measure.kernel_name
    assert f("void kgpu::k_tokenize_pool<false, false, false>(kgpu::PoolArgs)") == "k_tokenize_pool<false, false, false>"
    assert f("void kgpu::k_pack_write<true>(kgpu::PackArgs)") == "k_pack_write<true>"
    assert f("void kgpu::k_x<kgpu::Foo, 2>(kgpu::A)") == "k_x<kgpu::Foo, 2>"
    assert f("kgpu::k_compact(kgpu::BatchArgs)") == "k_compact" and f("void kgpu::dev::k_y<1>(int)") == "k_y<1>"
    assert f("k_plain") == "k_plain" and f("__amd_rocclr_copyBuffer") == "__amd_rocclr_copyBuffer"
    torch_name = ("void at::native::reduce_kernel<512, 1, at::native::ReduceOp<long, at::native::func_wrapper_t<long, at::native::sum_functor<long, long, long>"
                  "::operator()(at::TensorIterator&)::{lambda(long, long)#1}>, unsigned int, long, 4> >(at::native::ReduceOp<long>)")
    assert f(torch_name) == torch_name


def test_kernel_names_of_the_committed_profiles():
    assert STATS
    seen = set()
    for path in STATS:
        with open(path, newline="") as fh:
            names = [row["Name"] for row in csv.DictReader(fh)]
        short = [measure.kernel_name(n) for n in names]
        assert len(set(short)) == len(set(names)), path   # injective within a file
        for n, s in zip(names, short):
            if "kgpu::k_" in n:
                assert s.startswith("k_") and "(" not in s, (n, s)
            elif "reduce_kernel" in n:
                assert s == n
        seen.update(names)
    assert len(seen) == 29


# ---- 3. readers

def write_csv(path, cols, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(cols)
        w.writerows(rows)


def test_read_stats(tmp_path):
    d = str(tmp_path / "run")
    write_csv(os.path.join(d, "x", "y", "1_kernel_stats.csv"), ["Name", "Calls", "TotalDurationNs", "Percentage"],
              [["void kgpu::k_a<1>(int)", 3, 300, 50], ["kgpu::k_b(kgpu::A)", 2, 50, 10], ["void kgpu::k_a<1>(long)", 1, 100, 20], ["__amd_rocclr_copyBuffer", 4, 40, 20]])
    write_csv(os.path.join(d, "x", "z", "2_kernel_stats.csv"), ["Name", "Calls", "TotalDurationNs"], [["void kgpu::k_a<2>(int)", 4, 240], ["void kgpu::k_ab(int)", 1, 7]])
    ks = measure.read_stats(d)
    assert ks == {"k_a<1>": (4, 400.0), "k_b": (2, 50.0), "__amd_rocclr_copyBuffer": (4, 40.0), "k_a<2>": (4, 240.0), "k_ab": (1, 7.0)}
    assert measure.per_call(ks, "k_a") == 80.0 and measure.per_call(ks, "k_b") == 25.0   # every instantiation of the function, and no other function
    with pytest.raises(KeyError, match="k_c"):
        measure.per_call(ks, "k_c")
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    with pytest.raises(RuntimeError, match="empty"):
        measure.read_stats(empty)
    with pytest.raises(RuntimeError, match="empty"):
        measure.read_dispatches(empty)


def test_read_dispatches(tmp_path):
    d = str(tmp_path)
    write_csv(os.path.join(d, "h", "7_kernel_trace.csv"), ["Kernel_Name", "Start_Timestamp", "End_Timestamp"],
              [["void kgpu::k_a<1>(int)", 300, 330], ["kgpu::k_b(kgpu::A)", 200, 205], ["void kgpu::k_a<1>(int)", 100, 110], ["void kgpu::k_a<1>(int)", 1000, 1020]])
    assert measure.read_dispatches(d) == {"k_a<1>": [10, 30, 20], "k_b": [5]}


# ---- 4. the trace call

ROCPROF = """\
#!{python}
import os, subprocess, sys
a = sys.argv[1:]
flags = {flags!r}   # exactly these, then -d DIR -- <program ...>
n = len(flags)
assert a[:n] == flags and a[n] == "-d" and a[n + 2] == "--" and len(a) > n + 3, a
d, program = a[n + 1], a[n + 3:]
if {status}:
    sys.stderr.write("the profiler is in trouble\\n")
    sys.exit({status})
rc = subprocess.run(program).returncode
os.makedirs(os.path.join(d, "host", "1"))
if "--stats" in flags:
    with open(os.path.join(d, "host", "1", "1_kernel_stats.csv"), "w") as f:
        f.write('"Name","Calls","TotalDurationNs"\\n"void kgpu::k_a<2>(int)",2,500\\n')
else:   # per dispatch, out of order
    with open(os.path.join(d, "host", "1", "1_kernel_trace.csv"), "w") as f:
        f.write('"Kernel_Name","Start_Timestamp","End_Timestamp"\\n"void kgpu::k_a<2>(int)",50,57\\n"void kgpu::k_a<2>(int)",10,13\\n')
sys.exit(rc)
"""


def stand_in(tmp_path, monkeypatch, status, stats=True):
    exe = tmp_path / "bin" / "rocprofv3"
    exe.parent.mkdir()
    exe.write_text(ROCPROF.format(python=sys.executable, status=status, flags=["--kernel-trace", *(["--stats"] if stats else []), "--output-format", "csv"]))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("PATH", str(exe.parent) + os.pathsep + os.environ["PATH"])
    tool = tmp_path / "tool.py"
    tool.write_text("import sys; print('child', *sys.argv[1:])\n")
    return str(tool)


def test_trace(tmp_path, monkeypatch):
    tool = stand_in(tmp_path, monkeypatch, 0)
    assert measure.trace(tool, ["--leg", "trace-child"], 30) == ("child --leg trace-child\n", {"k_a<2>": (2, 500.0)})


def test_trace_per_dispatch(tmp_path, monkeypatch):
    tool = stand_in(tmp_path, monkeypatch, 0, stats=False)   # no --stats on the command line, and the per-dispatch reader
    assert measure.trace(tool, ["--leg", "kernel-child"], 30, stats=False) == ("child --leg kernel-child\n", {"k_a<2>": [3, 7]})


def test_trace_failure(tmp_path, monkeypatch):
    tool = stand_in(tmp_path, monkeypatch, 7)
    with pytest.raises(RuntimeError, match=r"\(7\).*the profiler is in trouble"):
        measure.trace(tool, [], 30)


# ---- 5. loops

class Clock:
    def __init__(self):
        self.t = 0

    def __call__(self):
        self.t += 1
        return self.t


def recording(names, calls):
    return {n: (lambda n=n: calls.append(n)) for n in names}


def test_summary():
    assert measure.summary([1, 2, 4]) == (2, 1.5)


def test_interleaved():
    calls = []
    out = measure.interleaved(recording("xy", calls), 2, 3, before=lambda: calls.append("before"), clock=Clock())
    assert calls == ["before", "x", "before", "y"] * 6
    assert out == {"x": [1, 1], "y": [1, 1]}   # (the counting clock: every call takes one tick)


def test_alternated():
    calls = []
    out = measure.alternated(recording("xy", calls), clock=Clock())
    assert calls == ["x", "y"] * 5 and out == {"x": [1] * 5, "y": [1] * 5}


def test_windows():
    calls = []
    out = measure.windows(recording("xy", calls), 4, 3, clock=Clock())
    assert calls == ["x"] * 4 + ["y"] * 4 + (["x"] * 4 + ["y"] * 4) * 3   # one warm-up window per arm, then alternated
    assert out == {"x": [0.25] * 3, "y": [0.25] * 3}


# ---- 6. the pipelined loop

class FakeContext:
    def __init__(self, name, log, k):
        self.name, self.log, self.k = name, log, k

    def sync(self):
        self.log.append(f"sync {self.name}")
        return 10 + self.k

    def sync_lines(self):
        self.log.append(f"sync_lines {self.name}")
        return 100 + self.k


ORDER = ["sync_lines c0", "submit c0 b0",
         "sync_lines c1", "submit c1 b1", "sync c0", "consume c0 b0",
         "sync_lines c2", "submit c2 b2", "sync c1", "consume c1 b1",
         "sync_lines c0", "submit c0 b3", "sync c2", "consume c2 b2",
         "sync c0", "consume c0 b3",
         "sync_lines c0", "sync_lines c1", "sync_lines c2"]


@pytest.mark.parametrize("with_consumer", [True, False])
def test_pipelined(with_consumer):
    log = []
    ctxs = [FakeContext(f"c{k}", log, k) for k in range(3)]

    def submit(c, slot, i):
        assert c is ctxs[slot]
        log.append(f"submit {c.name} b{i}")

    def consume(c, slot, j):
        assert c is ctxs[slot]
        log.append(f"consume {c.name} b{j}")

    dt, synced, lines = measure.pipelined(ctxs, 4, submit, consume if with_consumer else None, clock=Clock())
    assert log == [x for x in ORDER if with_consumer or not x.startswith("consume")]
    assert dt == 1 and synced == 10 + 11 + 12 + 10 and lines == (100 + 101 + 102 + 100) + (100 + 101 + 102)


# ---- 7. --help

@pytest.mark.parametrize("tool", PORTED)
def test_help(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip(), r.stderr
