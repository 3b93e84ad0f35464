#!/usr/bin/env python3
"""Static instruction count of one kernel instantiation, per phase of the pool kernel's sentence loop -- no GPU needed.

    python tools/pool_static_count.py [--src kanpyo_amd/csrc/kgpu_pool.hip] [--name 'k_tokenize_pool<false,false,false>'] [--asm listing.s] [--no-loops]

Compiles the .hip file to gfx950 assembly with the Makefile's CXXFLAGS plus -gline-tables-only (or reads a listing made that way: --asm), picks the
instantiation whose symbol holds --name (a template argument list of true / false is put into its mangled form), and prints

  * per phase the static instructions by class.  A phase is a range of source lines of the .hip file, found by the anchor text of its first line
    (PHASES below), so the table follows the source when lines move.  Classes go by opcode prefix alone: v_ (VALU), ds_ (LDS), global_ / flat_ /
    buffer_ / scratch_ (vector memory), s_load / s_buffer_load (scalar loads), s_branch / s_cbranch / s_setpc / s_endpgm (branches), s_waitcnt / s_nop
    (waits), every other s_ (SALU) -- and, beside them, the four exec-mask forms the compiler's bookkeeping of divergent control flow is made of;
  * the v_writelane_b32 / v_readlane_b32 (SGPR spill traffic, and the kernel's own lane reads) by source line;
  * the body of every innermost loop (a backward branch that encloses no other).

An instruction inlined from a header (or from a helper further up the file) carries that line, not the phase's: it is given to the phase it lies
INSIDE by position -- between the first and the last instruction of the phase's own lines in the listing -- the nearest own-line instruction in
front of it deciding between phases that overlap.  The count is static: what a sentence executes depends on the trip counts (profiles/pmc_*.json)."""
import argparse
import os
import re
import subprocess
import sys
from collections import Counter, OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (phase, text its first line holds), in source order; a phase ends where the next one starts
PHASES = [
    ("entry", "void k_tokenize_pool(PoolArgs)"),
    ("ticket/offsets", "for (uint32_t iter = 0;; ++iter)"),
    ("load", "const uint32_t tsh ="),
    ("reserve", "constexpr uint32_t MS ="),
    ("stage + carve", "---- phase 0a"),
    ("decode", "---- phase 0b"),
    ("walk", "---- phase 1:"),
    ("scan", "---- phase 2:"),
    ("3a", "---- phase 3:"),
    ("3b", "// 3b, lane = node"),
    ("3c", "const uint32_t lds0 ="),
    ("stage B", "---- phase 4:"),
    ("backtrace + tokens", "---- phase 5:"),
    ("exit", "}  // attempt"),
]
CLASSES = ["VALU", "LDS", "VMEM", "SMEM", "branch", "wait", "SALU"]
EXEC_FORMS = ["s_and_saveexec_b64", "s_or_b64", "s_andn2_b64", "s_cbranch_execz"]
LANE_OPS = ["v_writelane_b32", "v_readlane_b32"]


def classify(op):
    """instruction class of a mnemonic, by prefix; None: not an instruction of this target (a directive, a label)"""
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "SALU"
    return None


def mangled_fragment(name):
    """'k_tokenize_pool<false,true,false>' -> 'k_tokenize_poolILb0ELb1ELb0EE'; a name without '<' is taken as it is"""
    m = re.fullmatch(r"\s*([\w:]+)\s*<([^<>]*)>\s*", name)
    if not m:
        return name.strip()
    base = m.group(1).split("::")[-1]
    args = [a.strip() for a in m.group(2).split(",")]
    if not all(a in ("true", "false") for a in args):
        raise SystemExit(f"{name}: only template arguments true / false are translated; give a part of the mangled symbol instead")
    return base + "I" + "".join("Lb1E" if a == "true" else "Lb0E" for a in args) + "E"


def function_lines(asm_lines, fragment):
    """the listing lines of the one function whose symbol holds `fragment`: from its label to its .Lfunc_end"""
    syms = [m.group(1) for l in asm_lines for m in [re.match(r"\s*\.type\s+(\S+),@function", l)] if m]
    hits = [s for s in syms if fragment in s]
    if len(hits) != 1:
        raise SystemExit(f"{fragment!r} names {len(hits)} functions of {len(syms)}: {hits or syms}")
    start = next(i for i, l in enumerate(asm_lines) if l.startswith(hits[0] + ":"))
    end = next(i for i in range(start, len(asm_lines)) if asm_lines[i].startswith(".Lfunc_end"))
    return hits[0], asm_lines[start + 1:end]


def parse(fn_lines, main_name, files=None):
    """-> [(mnemonic, text, source line or None, labels in front of it)]: every instruction of the function in listing order; the source line is the
    .hip file's own (a line of another file, or line 0, is None).  `files`: file numbers known from earlier in the listing."""
    files = dict(files or {})
    out, cur, labels = [], None, []
    for l in fn_lines:
        s = l.split(";", 1)[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"\s*\.file\s+(\d+)\s+(?:\"[^\"]*\"\s+)?\"([^\"]*)\"", s)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = int(m.group(2)) if files.get(int(m.group(1))) == main_name and int(m.group(2)) > 0 else None
            continue
        m = re.match(r"([.\w$]+):\s*$", s)
        if m:
            labels.append(m.group(1))
            continue
        if s.lstrip().startswith("."):
            continue
        tok = s.split()
        if classify(tok[0]) is None:
            continue
        out.append((tok[0], " ".join(tok), cur, labels))
        labels = []
    return out


def phase_ranges(src_lines, phases=PHASES):
    """-> [(phase, first line, last line)] (1-based, inclusive) from the anchors; every anchor must be found once behind the one before it"""
    firsts, at = [], 0
    for name, anchor in phases:
        hit = next((i for i in range(at, len(src_lines)) if anchor in src_lines[i]), None)
        if hit is None:
            raise SystemExit(f"phase {name!r}: no line behind {at} holds {anchor!r}")
        firsts.append((name, hit + 1))
        at = hit + 1
    return [(n, f, (firsts[k + 1][1] - 1 if k + 1 < len(firsts) else len(src_lines))) for k, (n, f) in enumerate(firsts)]


def attribute(instrs, ranges):
    """-> the phase of every instruction.  Own-line instructions: the range their line is in.  The others: by position (module docstring)."""
    def of_line(ln):
        return next((n for n, f, t in ranges if f <= ln <= t), None)

    own = [of_line(ln) if ln is not None else None for _, _, ln, _ in instrs]
    first, last = {}, {}
    for i, p in enumerate(own):
        if p is not None:
            first.setdefault(p, i)
            last[p] = i
    nxt, follow = [None] * len(instrs), None
    for i in range(len(instrs) - 1, -1, -1):
        if own[i] is not None:
            follow = own[i]
        nxt[i] = follow
    out, prev = [], None
    for i, p in enumerate(own):
        if p is not None:
            prev = p
            out.append(p)
        elif prev is not None and i <= last[prev]:
            out.append(prev)          # inside the phase in front of it
        elif nxt[i] is not None:
            out.append(nxt[i])        # behind that phase's last own line: what follows encloses it
        else:
            out.append(prev or ranges[0][0])
    return out


def table(instrs, phases_of, ranges):
    rows = OrderedDict((n, Counter()) for n, _, _ in ranges)
    for (op, _, _, _), p in zip(instrs, phases_of):
        rows[p][classify(op)] += 1
        rows[p]["all"] += 1
        if op in EXEC_FORMS:
            rows[p][op] += 1
    return rows


def innermost_loops(instrs):
    """-> [(first index, last index)]: a backward branch to a label in front of it, enclosing no other such pair"""
    where = {lb: i for i, ins in enumerate(instrs) for lb in ins[3]}
    loops = []
    for i, (op, text, _, _) in enumerate(instrs):
        if classify(op) == "branch" and len(text.split()) > 1:
            t = where.get(text.split()[-1])
            if t is not None and t <= i:
                loops.append((t, i))
    return [(a, b) for a, b in loops if not any((c, e) != (a, b) and a <= c and e <= b for c, e in loops)]


def resources(asm_lines, sym):
    """the kernel's registers, scratch and spill counts from the listing's metadata (the figures `make resource-usage` prints)"""
    keys = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")
    at = next((i for i, l in enumerate(asm_lines) if re.match(r"\s+\.name:\s+" + re.escape(sym) + r"\s*$", l)), None)
    out = {}
    for l in asm_lines[at + 1:at + 12] if at is not None else []:
        m = re.match(r"\s+\.(\w+):\s+(\d+)\s*$", l)
        if m and m.group(1) in keys:
            out[m.group(1)] = int(m.group(2))
        elif re.match(r"\s+- \.", l):
            break
    return out


def render(rows, ranges):
    cols = ["all"] + CLASSES + EXEC_FORMS
    short = {"s_and_saveexec_b64": "saveexec", "s_or_b64": "or_b64", "s_andn2_b64": "andn2_b64", "s_cbranch_execz": "execz"}
    head = f"{'phase':<20}{'lines':>10}" + "".join(f"{short.get(c, c):>10}" for c in cols)
    lines = [head]
    tot = Counter()
    for n, f, t in ranges:
        lines.append(f"{n:<20}{f'{f}-{t}':>10}" + "".join(f"{rows[n][c]:>10}" for c in cols))
        tot.update(rows[n])
    lines.append(f"{'whole kernel':<20}{'':>10}" + "".join(f"{tot[c]:>10}" for c in cols))
    return "\n".join(lines)


def makefile_flags(csrc):
    for l in open(os.path.join(csrc, "Makefile"), encoding="utf-8"):
        m = re.match(r"CXXFLAGS\s*\?=\s*(.*)", l)
        if m:
            return m.group(1).split()
    raise SystemExit("the Makefile sets no CXXFLAGS")


def compile_asm(src, extra):
    csrc = os.path.dirname(os.path.abspath(src))
    cmd = [HIPCC, "--offload-arch=gfx950"] + makefile_flags(csrc) + extra + ["-gline-tables-only", "-S", "--cuda-device-only", os.path.basename(src), "-o", "-"]
    return subprocess.run(cmd, cwd=csrc, check=True, capture_output=True, text=True).stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_pool.hip"))
    ap.add_argument("--name", default="k_tokenize_pool<false,false,false>")
    ap.add_argument("--asm", help="a listing made with -gline-tables-only -S --cuda-device-only (instead of compiling)")
    ap.add_argument("--extra", default="", help="further compiler flags, as the Makefile's EXTRA")
    ap.add_argument("--no-loops", action="store_true")
    a = ap.parse_args()
    asm = open(a.asm, encoding="utf-8").read() if a.asm else compile_asm(a.src, a.extra.split())
    asm_lines = asm.splitlines()
    sym, fn = function_lines(asm_lines, mangled_fragment(a.name))
    main_name = os.path.basename(a.src)
    # (file numbers are declared where first used, possibly in an earlier function of the listing)
    files = {int(m.group(1)): os.path.basename(m.group(2)) for l in asm_lines for m in [re.match(r"\s*\.file\s+(\d+)\s+(?:\"[^\"]*\"\s+)?\"([^\"]*)\"", l)] if m}
    instrs = parse(fn, main_name, files)
    ranges = phase_ranges(open(a.src, encoding="utf-8").read().splitlines())
    ph = attribute(instrs, ranges)
    print(f"{sym}: {len(instrs)} static instructions")
    res = resources(asm_lines, sym)
    if res:
        print(f"VGPRs {res.get('vgpr_count')}  SGPRs {res.get('sgpr_count')}  scratch {res.get('private_segment_fixed_size')} bytes/lane  "
              f"SGPR spills {res.get('sgpr_spill_count')}  VGPR spills {res.get('vgpr_spill_count')}")
    print(render(table(instrs, ph, ranges), ranges))
    for op in LANE_OPS:
        by = Counter((ln if ln is not None else 0) for o, _, ln, _ in instrs if o == op)
        print(f"\n{op}: {sum(by.values())}  (source line: count; 0 = a line of another file)")
        print("  " + "  ".join(f"{ln}: {c}" for ln, c in sorted(by.items())))
    if not a.no_loops:
        for lo, hi in innermost_loops(instrs):
            lines = sorted({ln for _, _, ln, _ in instrs[lo:hi + 1] if ln is not None})
            print(f"\ninnermost loop, {hi - lo + 1} instructions, phase {ph[lo]}, lines {lines[0] if lines else '?'}-{lines[-1] if lines else '?'}:")
            for op, text, ln, labels in instrs[lo:hi + 1]:
                for lb in labels:
                    print(f"  {lb}:")
                print(f"    {text:<64}; {ln if ln is not None else '-'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
