"""The model inputs (include/kanpyo_gpu.h, "model inputs") without a device: kgpu_pack_host against the plain-Python rule of tests/pack_ref.py on a
seeded sweep of the shapes at which the rule changes; both against the `tokenizers` library's truncation and template processing; the hand-checkable
fixture; the argument errors, the capacity protocol and the bad offsets of rules 6 to 8; the new symbols; and kgpu_pack_host in a stand-alone program
under AddressSanitizer + UBSan."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pack_ref as P
from conftest import ROOT, load_golden
from kanpyo_amd import _lib
from kanpyo_amd.pack import pack_host, pack_opts, sample_of_row
from pack_cases import ragged, sweep_calls

INC = os.path.join(ROOT, "include")
ROW_KEYS = ("input_ids", "token_type_ids", "attention_mask", "spans", "token_index", "row_offsets", "status")
SWEEP_LENGTHS = (3, 4, 5, 7, 8, 16, 17, 64, 65, 512)


def run_both(ids, ranges_a, ranges_b, spans, tix, **o):
    """One call of kgpu_pack_host and of the reference over the same lists -> (host dict, reference dict as arrays)."""
    opts = pack_opts(o["max_length"], o.get("stride", 0), o["strategy"], o.get("windows", True), o.get("cls_id", 101), o.get("sep_id", 102), o.get("pad_id", 0),
                     o.get("trim_front", 0), o.get("trim_back", 0))
    ref = P.pack(ids, ranges_a, ids if ranges_b is not None else None, ranges_b, spans_in=spans, tix_in=tix,
                 **{k: o[k] for k in ("max_length", "stride", "strategy", "windows", "cls_id", "sep_id", "pad_id", "trim_front", "trim_back") if k in o})
    got = pack_host(opts, np.array(ids, dtype=np.int64).astype(np.int32), np.array(ranges_a, dtype=np.uint64), None,
                    None if ranges_b is None else np.array(ranges_b, dtype=np.uint64), np.array(spans, dtype=np.uint32).reshape(-1, 4), np.array(tix, dtype=np.int32))
    return got, P.as_arrays(ref, o["max_length"])


def assert_same(got, want, what):
    for k in ROW_KEYS:
        g = got[k]
        if k == "spans":
            g = np.ascontiguousarray(g).view(np.uint32).reshape(want[k].shape)
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k)


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_reference_writes_and_what_the_library_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pack_fixture.py"), "--print"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "fixture_pack.json"), encoding="utf-8") as f:
        assert f.read() == r.stdout, "tests/golden/fixture_pack.json is not what tools/gen_pack_fixture.py writes"
    cases = load_golden("fixture_pack.json")["cases"]
    names = {c["name"] for c in cases}
    assert {"only_second_three_windows_rule5", "longest_first_rule4_short_side_kept", "longest_first_rule4_both_beyond_room",
            "longest_first_rule4_short_side_past_half"} <= names
    for c in cases:
        o = dict(c["opts"])
        o["strategy"] = {v: k for k, v in P.STRATEGY_NAMES.items()}[o["strategy"]]
        got, _ = run_both(c["ids"], c["off_a"], c["off_b"], [tuple(s) for s in c["spans_in"]], c["tix_in"], **o)
        want = P.as_arrays({k: c[k] for k in ROW_KEYS}, o["max_length"])
        assert_same(got, want, c["name"])
    three = next(c for c in cases if c["name"] == "only_second_three_windows_rule5")
    assert three["row_offsets"] == [0, 3] and [row[4] for row in three["input_ids"]] == [60, 63, 66]   # the windows start 3 apart, sharing 2


# ---- 2. pack_host == pack_ref on the sweep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length", SWEEP_LENGTHS)
def test_host_equals_reference_on_the_sweep(max_length):
    rng = random.Random(1000 + max_length)
    seen, trims, calls = {P.OK: 0, P.CUT: 0, P.NO_ROOM: 0}, set(), 0
    multi_row = step_one = 0
    for o, la, lb in sweep_calls(max_length, rng, samples_per_call=None if max_length <= 65 else 8):
        ids, off_a, off_b, spans, tix = ragged(rng, la, lb)
        got, want = run_both(ids, off_a, off_b, spans, tix, **o)
        assert_same(got, want, o)
        for s in want["status"].tolist():
            seen[s] += 1
        rows = np.diff(want["row_offsets"].astype(np.int64))
        multi_row += int((rows > 1).sum())
        step_one += int((rows > 2 * (max_length - 3)).sum())
        assert np.array_equal(sample_of_row(got["row_offsets"]), np.repeat(np.arange(len(la)), rows))
        trims.add((o["trim_front"], o["trim_back"]))
        calls += 1
    assert calls >= 10 and trims == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert seen[P.OK] > 0 and seen[P.CUT] > 0, seen
    if max_length > 3:   # (max_length 3 is singles with room 1: a fixed side never takes the room)
        assert seen[P.NO_ROOM] > 0 and multi_row > 0, (seen, multi_row)
    if max_length >= 7:
        assert step_one > 0   # stride = w - 1 over 3 x room: more than 2 x room rows from one sample


def test_ranges_need_not_abut_and_both_id_arrays_are_indexed_by_the_same_offsets():
    """Rule 8: offsets are taken as they are.  Separate a and b arrays whose ranges overlap, repeat and leave gaps."""
    rng = random.Random(77)
    ids = [rng.randrange(-2**31, 2**31) for _ in range(40)]
    ids_b = [rng.randrange(-2**31, 2**31) for _ in range(40)]
    off_a, off_b = [3, 3, 9, 9, 40], [38, 40, 40, 40, 40]   # sample 0: a empty, b two long; sample 3: a = [9, 40), b empty
    opts = pack_opts(8, 1, "only_first", True, 1, 2, 0)
    got = pack_host(opts, np.array(ids, dtype=np.int64).astype(np.int32), np.array(off_a, dtype=np.uint64), np.array(ids_b, dtype=np.int64).astype(np.int32),
                    np.array(off_b, dtype=np.uint64))
    ref = P.pack(ids, off_a, ids_b, off_b, max_length=8, stride=1, strategy=P.ONLY_FIRST, windows=True, cls_id=1, sep_id=2, pad_id=0)
    assert got["input_ids"].tolist() == ref["input_ids"] and got["token_type_ids"].tolist() == ref["token_type_ids"]
    assert got["row_offsets"].tolist() == ref["row_offsets"] and got["status"].tolist() == ref["status"] and "spans" not in got and "token_index" not in got


# ---- 3. against the tokenizers library ----------------------------------------------------------------------------------------------------------------
def test_reference_and_host_equal_the_tokenizers_library():
    tk = pytest.importorskip("tokenizers")
    from tokenizers import models, pre_tokenizers, processors

    V = 400
    vocab = {str(i): i for i in range(V)}
    vocab.update({"CLS": V, "SEP": V + 1, "PAD": V + 2, "UNK": V + 3})
    cls_id, sep_id, pad_id = V, V + 1, V + 2
    rng = random.Random(2024)
    drawn_multi = drawn_cut = compared_multi = compared_cut = 0
    N = 3000
    for case in range(N):
        max_length = rng.randint(4, 24)
        pair = rng.random() < 0.6
        ns = 3 if pair else 2
        room = max_length - ns
        if room < 1:
            pair, ns, room = False, 2, max_length - 2
        strategy = rng.choice((P.LONGEST_FIRST, P.ONLY_FIRST, P.ONLY_SECOND) if pair else (P.LONGEST_FIRST, P.ONLY_FIRST))
        La, Lb = rng.randint(0, 30), (rng.randint(0, 30) if pair else 0)
        fits = La + Lb <= room
        if not fits and strategy != P.LONGEST_FIRST:   # inside the library's domain: w >= 1 (it rejects what the rule reports as NO_ROOM)
            fixed_max = room - 1
            if strategy == P.ONLY_FIRST:
                Lb = min(Lb, fixed_max)
                La = max(La, room - Lb + 1)
            else:
                La = min(La, fixed_max)
                Lb = max(Lb, room - La + 1)
        w = room if fits or strategy == P.LONGEST_FIRST else room - (Lb if strategy == P.ONLY_FIRST else La)
        limit = min(w, max_length - 3)
        stride = rng.randrange(limit) if limit >= 1 else 0
        a = [rng.randrange(V) for _ in range(La)]
        b = [rng.randrange(V) for _ in range(Lb)]
        lib_stride = 0 if strategy == P.LONGEST_FIRST else stride
        ids, off_a, off_b = a + b, [0, La], ([La, La + Lb] if pair else None)
        o = dict(max_length=max_length, stride=stride, strategy=strategy, windows=strategy != P.LONGEST_FIRST, cls_id=cls_id, sep_id=sep_id, pad_id=pad_id)
        ref = P.pack(ids, off_a, ids if pair else None, off_b, **o)
        got = pack_host(pack_opts(max_length, stride, strategy, o["windows"], cls_id, sep_id, pad_id), np.array(ids, dtype=np.int32), np.array(off_a, dtype=np.uint64),
                        None, None if not pair else np.array(off_b, dtype=np.uint64))
        assert ref["status"][0] != P.NO_ROOM, "the generator left the library's domain"
        rows = len(ref["input_ids"])
        drawn_multi += rows > 1
        drawn_cut += ref["status"][0] == P.CUT and strategy == P.LONGEST_FIRST

        t = tk.Tokenizer(models.WordLevel(vocab, unk_token="UNK"))
        t.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
        t.post_processor = processors.TemplateProcessing(single="CLS $A SEP", pair="CLS $A SEP $B:1 SEP:1", special_tokens=[("CLS", cls_id), ("SEP", sep_id)])
        t.enable_truncation(max_length, stride=lib_stride, strategy=P.STRATEGY_NAMES[strategy])
        t.enable_padding(length=max_length, pad_id=pad_id, pad_token="PAD")
        text_a, text_b = " ".join(map(str, a)), " ".join(map(str, b))
        enc = t.encode(text_a, text_b) if pair else t.encode(text_a)   # (must not raise: the condition of this test)
        encs = [enc] if strategy == P.LONGEST_FIRST else [enc] + list(enc.overflowing)
        assert len(encs) == rows, (case, o, La, Lb, len(encs), rows)
        for k, e in enumerate(encs):
            assert list(e.ids) == ref["input_ids"][k] == got["input_ids"][k].tolist(), (case, o, La, Lb, k)
            assert list(e.type_ids) == ref["token_type_ids"][k] == got["token_type_ids"][k].tolist(), (case, o, La, Lb, k)
            assert list(e.attention_mask) == ref["attention_mask"][k] == got["attention_mask"][k].tolist(), (case, o, La, Lb, k)
        compared_multi += rows > 1
        compared_cut += ref["status"][0] == P.CUT and strategy == P.LONGEST_FIRST
    assert compared_multi >= drawn_multi > N // 4 and compared_cut >= drawn_cut > N // 10, (drawn_multi, drawn_cut)


# ---- 4. rules 6, 7, 8 -----------------------------------------------------------------------------------------------------------------------------------
def raw_call(opts, n, ids, off_a, off_b=None, n_in=None, rows=4, input_ids=True, spans_in=None, spans_out=None, tix_in=None, tix_out=None, status=True,
             row_offsets=True, off_a_ptr=None, ids_ptr=None, input_ptr=None):
    L = _lib.lib()
    ML = max(int(opts.max_length), 1) if opts is not None else 8
    out = np.full((rows, ML), 0x5A5A5A5A, dtype=np.int32)
    roff, st, got = np.zeros(n + 2, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint8), C.c_uint64(0)
    rc = L.kgpu_pack_host(C.byref(opts) if opts is not None else None, n, ids_ptr if ids_ptr is not None else ids.ctypes.data,
                          off_a_ptr if off_a_ptr is not None else off_a.ctypes.data, ids.ctypes.data if off_b is not None else None,
                          off_b.ctypes.data if off_b is not None else None, ids.size if n_in is None else n_in,
                          spans_in, tix_in, (input_ptr if input_ptr is not None else out.ctypes.data) if input_ids else None, None, None, spans_out, tix_out, rows,
                          roff.ctypes.data if row_offsets else None, st.ctypes.data if status else None, C.byref(got))
    return rc, int(got.value), out, roff, st


def test_argument_errors_of_rule_6():
    ids, off = np.arange(10, dtype=np.int32), np.array([0, 4, 10], dtype=np.uint64)
    INV = _lib.KGPU_ERR_INVALID_ARG
    ok = pack_opts(8, 1, "only_first")
    assert raw_call(ok, 2, ids, off)[0] == _lib.KGPU_OK
    assert raw_call(None, 2, ids, off)[0] == INV
    for bad in (pack_opts(2, 0, "only_first"), pack_opts(65537, 0, "only_first"), pack_opts(8, 6, "only_first"), pack_opts(8, 0, 3), pack_opts(8, 0, "longest_first", True),
                pack_opts(8, 0, "only_second"), pack_opts(8, 0, "only_first", trim_front=2), pack_opts(8, 0, "only_first", trim_back=2)):
        assert raw_call(bad, 2, ids, off)[0] == INV, [getattr(bad, f) for f, _ in bad._fields_]
    assert raw_call(pack_opts(3, 0, "only_first"), 2, ids, off, rows=16)[0] == _lib.KGPU_OK             # ns + 1 for singles ...
    assert raw_call(pack_opts(3, 0, "only_first"), 2, ids, off, off_b=off)[0] == INV                   # ... is below ns + 1 for pairs
    assert raw_call(pack_opts(4, 0, "only_second"), 2, ids, off, off_b=off)[0] == _lib.KGPU_OK
    assert raw_call(pack_opts(8, 5, "only_first"), 2, ids, off)[0] == _lib.KGPU_OK and raw_call(pack_opts(8, 5, "only_first"), 2, ids, off, off_b=off)[0] == INV
    assert raw_call(pack_opts(65536, 0, "only_first"), 0, ids, off, rows=0)[0] == _lib.KGPU_OK
    flags = pack_opts(8, 0, "only_first")
    flags.flags = 2
    small = pack_opts(8, 0, "only_first")
    small.size -= 4
    assert raw_call(flags, 2, ids, off)[0] == INV and raw_call(small, 2, ids, off)[0] == INV
    # null and misaligned pointers; spans out without spans in
    assert raw_call(ok, 2, ids, off, input_ids=False)[0] == INV and raw_call(ok, 2, ids, off, status=False)[0] == INV and raw_call(ok, 2, ids, off, row_offsets=False)[0] == INV
    assert raw_call(ok, 2, ids, off, ids_ptr=ids.ctypes.data + 2)[0] == INV and raw_call(ok, 2, ids, off, off_a_ptr=off.ctypes.data + 4)[0] == INV
    scratch = np.zeros(64, dtype=np.int32)
    assert raw_call(ok, 2, ids, off, input_ptr=scratch.ctypes.data + 1)[0] == INV
    sp = np.zeros(16 * 12 + 16, dtype=np.uint8)
    base = sp.ctypes.data + (-sp.ctypes.data) % 16
    assert raw_call(ok, 2, ids, off, spans_out=base)[0] == INV                                  # out without in
    assert raw_call(ok, 2, ids, off, spans_in=base + 4, spans_out=None)[0] == INV               # misaligned
    assert raw_call(ok, 2, ids, off, tix_out=scratch.ctypes.data)[0] == INV                     # token indices out without in
    assert raw_call(ok, 2, ids, off, spans_in=base)[0] == _lib.KGPU_OK                          # in without out: carried nowhere, no error
    with pytest.raises(ValueError):
        pack_opts(8, 0, "left")


def test_capacity_protocol_of_rule_7():
    rng = random.Random(5)
    ids = np.array([rng.randrange(1000) for _ in range(60)], dtype=np.int32)
    off = np.array([0, 30, 31, 60], dtype=np.uint64)
    opts = pack_opts(8, 2, "only_first", True, 1, 2, 0)
    full = pack_host(opts, ids, off)
    R = int(full["row_offsets"][-1])
    assert R == full["input_ids"].shape[0] >= 10
    rc, got, out, roff, st = raw_call(opts, 3, ids, off, rows=R + 1)
    assert rc == _lib.KGPU_OK and got == R and np.array_equal(out[:R], full["input_ids"]) and (out[R] == 0x5A5A5A5A).all()   # the row behind the last is untouched
    rc, got, out, roff, st = raw_call(opts, 3, ids, off, rows=R - 1)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == R and (out == 0x5A5A5A5A).all()
    assert roff[:4].tolist() == full["row_offsets"].tolist() and st[:3].tolist() == full["status"].tolist()   # always written
    with pytest.raises(_lib.KgpuError) as e:
        pack_host(opts, ids, off, row_capacity=R - 1)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and e.value.rows == R
    assert pack_host(opts, ids, off, row_capacity=R + 3)["input_ids"].shape == (R, 8)
    empty = pack_host(opts, ids, np.array([0], dtype=np.uint64))
    assert empty["input_ids"].shape == (0, 8) and empty["row_offsets"].tolist() == [0] and empty["status"].size == 0


def test_bad_offsets_of_rule_8():
    ids = np.arange(10, dtype=np.int32)
    opts = pack_opts(8, 0, "only_first")
    INV = _lib.KGPU_ERR_INVALID_ARG
    for off in ([0, 4, 11], [4, 0, 10], [0, 2**63, 10], [2**64 - 1, 2, 10]):
        rc, _, out, _, _ = raw_call(opts, 2, ids, np.array(off, dtype=np.uint64))
        assert rc == INV and (out == 0x5A5A5A5A).all(), off
    good = np.array([0, 4, 10], dtype=np.uint64)
    for off_b in ([0, 4, 11], [10, 9, 10], [0, 0, 2**40]):
        assert raw_call(pack_opts(8, 0, "only_second"), 2, ids, good, off_b=np.array(off_b, dtype=np.uint64))[0] == INV, off_b
    assert raw_call(opts, 2, ids, good, n_in=9)[0] == INV          # past n_ids_in, though inside the array
    assert raw_call(opts, 2, ids, np.array([10, 10, 10], dtype=np.uint64))[0] == _lib.KGPU_OK   # empty ranges at the very end are ranges
    with pytest.raises(_lib.KgpuError):
        pack_host(opts, ids, np.array([0, 4, 11], dtype=np.uint64))


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_struct_and_constants(tmp_path):
    L = _lib.lib()
    header = open(os.path.join(INC, "kanpyo_gpu.h"), encoding="utf-8").read()
    for s in ("kgpu_pack_host", "kgpu_pack_device"):
        assert s in _lib.SYMBOLS and hasattr(L, s) and getattr(L, s).argtypes and s + "(" in header, s
    assert len(L.kgpu_pack_device.argtypes) == 18 and len(L.kgpu_pack_host.argtypes) == 18
    src = tmp_path / "pack_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kanpyo_gpu.h"\nint main(void) {\n'
                   ' printf("%zu", sizeof(kgpu_pack_opts));\n'
                   + "".join(f' printf(" %zu", offsetof(kgpu_pack_opts, {f}));\n' for f, _ in _lib.PackOpts._fields_)
                   + ' printf(" %u %u %u %u %d %d %d\\n", KGPU_PACK_WINDOWS, KGPU_PACK_LONGEST_FIRST, KGPU_PACK_ONLY_FIRST, KGPU_PACK_ONLY_SECOND, KGPU_PACK_OK, KGPU_PACK_CUT,'
                   " KGPU_PACK_NO_ROOM);\n return 0;\n}\n")
    exe = str(tmp_path / "pack_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, str(src), "-o", exe], check=True)
    nums = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P_ = _lib.PackOpts
    assert nums[0] == C.sizeof(P_) == 40 and nums[1:11] == [getattr(P_, f).offset for f, _ in P_._fields_]
    assert nums[11:] == [_lib.KGPU_PACK_WINDOWS, _lib.KGPU_PACK_LONGEST_FIRST, _lib.KGPU_PACK_ONLY_FIRST, _lib.KGPU_PACK_ONLY_SECOND, _lib.KGPU_PACK_OK, _lib.KGPU_PACK_CUT,
                         _lib.KGPU_PACK_NO_ROOM] == [P.WINDOWS, P.LONGEST_FIRST, P.ONLY_FIRST, P.ONLY_SECOND, P.OK, P.CUT, P.NO_ROOM]
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_pack.hip") == 2 and "kgpu_pack_rule.cpp" in mk and "kgpu_pack_host.cpp" in mk   # SRCS and the resource-usage target
    import kanpyo_amd
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.vocab import Vocab

    assert kanpyo_amd.pack_host is pack_host and callable(DeviceContext.pack) and callable(Vocab.encode_pairs_tensor)


# ---- 6. the host rule under the sanitizers, in a program of its own ---------------------------------------------------------------------------------------
def test_pack_host_under_asan_ubsan_in_a_standalone_program(tmp_path):
    exe = str(tmp_path / "pack_sanitize")
    csrc = os.path.join(ROOT, "kanpyo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC,
                        os.path.join(ROOT, "tests", "c_abi", "pack_sanitize.cpp"), os.path.join(csrc, "kgpu_pack_rule.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.startswith("pack sanitized ok "), (r.stdout[-500:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    calls, rows = (int(x) for x in r.stdout.split()[3:5])
    assert calls > 1000 and rows > 50000
