"""tools/pool_static_count.py on a dozen hand-written assembly lines: the classes by opcode prefix, the phase of an own-line instruction, the phase
BY POSITION of an instruction that carries a header's line, the lane-op counts' source lines and the innermost loop."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("pool_static_count", os.path.join(ROOT, "tools", "pool_static_count.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)

# a "source" of 12 lines: phase one = lines 2-5, phase two = lines 6-9, phase three = lines 10-12
SRC = ["// top", "// ONE", "a", "b", "c", "// TWO", "d", "e", "f", "// THREE", "g", "h"]
PHASES = [("one", "// ONE"), ("two", "// TWO"), ("three", "// THREE")]

ASM = """\
	.type	_ZN1k4kernILb0ELb1EEEvv,@function
_ZN1k4kernILb0ELb1EEEvv:                ; @_ZN1k4kernILb0ELb1EEEvv
.Lfunc_begin0:
	.file	0 "/somewhere" "kern.hip" md5 0x00
	.file	2 "." "helper.h"
	.loc	0 3 5 prologue_end              ; kern.hip:3:5
	s_load_dwordx2 s[4:5], s[0:1], 0x10
	.loc	2 40 1                          ; helper.h:40:1 @[ kern.hip:4:9 ]
	v_readfirstlane_b32 s6, v0
	s_waitcnt lgkmcnt(0)
	.loc	0 5 1                           ; kern.hip:5:1
	v_writelane_b32 v40, s6, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	.loc	0 7 1                           ; kern.hip:7:1
	ds_read_b32 v1, v2
	.loc	2 12 1                          ; helper.h:12:1
	v_add_u32_e32 v1, v1, v3
	s_and_saveexec_b64 s[8:9], vcc
	.loc	0 8 3 is_stmt 0                 ; kern.hip:8:3
	global_store_dword v4, v1, s[4:5]
	s_cbranch_execz .LBB0_1
; %bb.2:
	.loc	2 90 1                          ; helper.h:90:1
	s_or_b64 exec, exec, s[8:9]
	.loc	0 11 1                          ; kern.hip:11:1
	v_readlane_b32 s7, v40, 0
	.loc	0 0 1                           ; kern.hip:0:1
	s_nop 0
	s_endpgm
.Lfunc_end0:
	.size	_ZN1k4kernILb0ELb1EEEvv, .Lfunc_end0-_ZN1k4kernILb0ELb1EEEvv
"""


def _parsed():
    sym, fn = T.function_lines(ASM.splitlines(), T.mangled_fragment("k::kern<false,true>"))
    assert sym == "_ZN1k4kernILb0ELb1EEEvv"
    return T.parse(fn, "kern.hip")


def test_classes_by_prefix():
    want = {"v_add_u32_e32": "VALU", "v_writelane_b32": "VALU", "ds_read_b32": "LDS", "ds_bpermute_b32": "LDS", "global_load_dword": "VMEM",
            "flat_load_dword": "VMEM", "s_load_dwordx2": "SMEM", "s_buffer_load_dword": "SMEM", "s_branch": "branch", "s_cbranch_execz": "branch",
            "s_endpgm": "branch", "s_waitcnt": "wait", "s_nop": "wait", "s_and_saveexec_b64": "SALU", "s_or_b64": "SALU", "s_add_u32": "SALU",
            ".loc": None, ".LBB0_1:": None}
    assert {op: T.classify(op) for op in want} == want


def test_mangled_fragment():
    assert T.mangled_fragment("k_tokenize_pool<false,false,false>") == "k_tokenize_poolILb0ELb0ELb0EE"
    assert T.mangled_fragment("k_tokenize_poolILb1E") == "k_tokenize_poolILb1E"


def test_instructions_and_their_own_lines():
    ins = _parsed()
    assert [(op, ln) for op, _, ln, _ in ins] == [
        ("s_load_dwordx2", 3), ("v_readfirstlane_b32", None), ("s_waitcnt", None), ("v_writelane_b32", 5), ("ds_read_b32", 7), ("v_add_u32_e32", None),
        ("s_and_saveexec_b64", None), ("global_store_dword", 8), ("s_cbranch_execz", 8), ("s_or_b64", None), ("v_readlane_b32", 11), ("s_nop", None),
        ("s_endpgm", None)]
    assert ins[4][3] == [".LBB0_1"] and ins[4][1] == "ds_read_b32 v1, v2"   # the label sits on the instruction behind it; comments are dropped


def test_phase_ranges_follow_the_anchors():
    assert T.phase_ranges(SRC, PHASES) == [("one", 2, 5), ("two", 6, 9), ("three", 10, 12)]


def test_attribution_by_line_and_by_position():
    ins = _parsed()
    ph = T.attribute(ins, T.phase_ranges(SRC, PHASES))
    assert ph == ["one",      # line 3
                  "one",      # helper.h between phase one's first (line 3) and last (line 5) own instruction
                  "one",
                  "one",      # line 5
                  "two",      # line 7
                  "two",      # helper.h inside phase two
                  "two",
                  "two",      # line 8
                  "two",
                  "three",    # helper.h BEHIND phase two's last own instruction: the phase that follows encloses it
                  "three",    # line 11
                  "three",    # line 0 behind the last own line of all: stays with the phase in front
                  "three"]
    rows = T.table(ins, ph, T.phase_ranges(SRC, PHASES))
    assert rows["one"] == {"SMEM": 1, "VALU": 2, "wait": 1, "all": 4}
    assert rows["two"] == {"LDS": 1, "VALU": 1, "SALU": 1, "VMEM": 1, "branch": 1, "all": 5, "s_and_saveexec_b64": 1, "s_cbranch_execz": 1}
    assert rows["three"] == {"SALU": 1, "VALU": 1, "wait": 1, "branch": 1, "all": 4, "s_or_b64": 1}
    text = T.render(rows, T.phase_ranges(SRC, PHASES))
    assert text.splitlines()[-1].split()[:3] == ["whole", "kernel", "13"]


def test_innermost_loop():
    ins = _parsed()
    assert T.innermost_loops(ins) == [(4, 8)]
