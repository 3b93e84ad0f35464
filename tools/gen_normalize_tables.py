#!/usr/bin/env python3
"""The tables of the text normaliser (include/kanpyo_gpu.h, "text normalisation"), derived from Python's unicodedata alone.

    python tools/gen_normalize_tables.py                 # writes kanpyo_amd/csrc/kgpu_normalize_data.inc
    python tools/gen_normalize_tables.py --out DIR       # ... into DIR instead (the regeneration test)
    python tools/gen_normalize_tables.py --fixture       # writes tests/golden/fixture_normalize.json as well

The build never runs this: the generated file is committed, and tests/test_normalize_cpu.py compares it with a fresh run byte for byte whenever
the running Python carries the Unicode version the file names.  No file is read, nothing comes from a network.

The committed file is compact -- runs of code points with equal property bits, the decompositions by code point (build_tables says how) -- and
kgpu_normalize_table.cpp expands it, when the library is loaded, into the two-stage table, the decomposition index and the pool that
kgpu_normalize_core.h describes and the kernels read.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import unicodedata as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CP = 0x110000
BLOCK = 128
MAX_SEGMENT = 64          # KGPU_NORMALIZE_MAX_SEGMENT
S_BASE, L_BASE, V_BASE, T_BASE, L_COUNT, V_COUNT, T_COUNT = 0xAC00, 0x1100, 0x1161, 0x11A7, 19, 21, 28
S_COUNT = L_COUNT * V_COUNT * T_COUNT
FORMS = {"NFC": "NFD", "NFKC": "NFKD"}   # a form and its decomposition


def is_scalar(cp: int) -> bool:
    return not 0xD800 <= cp <= 0xDFFF


def is_hangul_syllable(cp: int) -> bool:
    return S_BASE <= cp < S_BASE + S_COUNT


def is_jamo_vt(cp: int) -> bool:
    return 0x1161 <= cp <= 0x1175 or 0x11A8 <= cp <= 0x11C2


def composition_pairs() -> dict:
    """(first, second) -> composite for exactly the code points with a two-member canonical decomposition and NFC(NFD(c)) == c (Hangul is arithmetic)."""
    pairs = {}
    for cp in range(MAX_CP):
        if not is_scalar(cp) or is_hangul_syllable(cp):
            continue
        d = U.decomposition(chr(cp))
        if not d or d.startswith("<"):
            continue
        parts = [int(x, 16) for x in d.split()]
        if len(parts) == 2 and U.normalize("NFC", U.normalize("NFD", chr(cp))) == chr(cp):
            pairs[(parts[0], parts[1])] = cp
    return pairs


_PAIRS = None
_SECONDS = None


def pairs_and_seconds():
    global _PAIRS, _SECONDS
    if _PAIRS is None:
        _PAIRS = composition_pairs()
        _SECONDS = {b for _, b in _PAIRS}
    return _PAIRS, _SECONDS


def boundary_before(cp: int, form: str) -> bool:
    """The definition of include/kanpyo_gpu.h: ccc(c) == 0, and the first code point f of c's full decomposition under the form has ccc 0, is the
    second member of no composition pair and is no Hangul V or T jamo."""
    if not is_scalar(cp):
        return True
    _, seconds = pairs_and_seconds()
    ch = chr(cp)
    if U.combining(ch):
        return False
    f = U.normalize(FORMS[form], ch)[0]
    return U.combining(f) == 0 and ord(f) not in seconds and not is_jamo_vt(ord(f))


def segments(text: str, form: str):
    """The segments of a line: one starts at the first code point and at every boundary."""
    start = 0
    for i in range(1, len(text)):
        if boundary_before(ord(text[i]), form):
            yield text[start:i]
            start = i
    if text:
        yield text[start:]


def normalize_line(data: bytes, form: str):
    """-> (bytes, status) by the rules of the header, through unicodedata: status 1 (not UTF-8) and 4 (a segment of more than its first code point and
    MAX_SEGMENT further ones after decomposition) leave the line as it is."""
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        return data, 1
    for seg in segments(text, form):
        if len(U.normalize(FORMS[form], seg)) > MAX_SEGMENT + 1:
            return data, 4
    return U.normalize(form, text).encode("utf-8"), 0


def build_tables():
    """The compact form the committed file holds (kgpu_normalize_table.cpp expands it when the library is loaded):
      runs   (first code point, property bits 0-12) of every run of code points with equal bits, ascending
      dec    per code point with a decomposition, ascending: (code point, NFD offset << 8 | length, NFKD offset << 8 | length) into pool; length 0: itself
      pool   the decompositions' code points, each sequence stored once
      comp   (first << 21 | second, composite) of the primary composition pairs, ascending"""
    pairs, seconds = pairs_and_seconds()
    for (a, _), c in pairs.items():
        assert U.combining(chr(a)) == 0 and U.combining(chr(c)) == 0, "a primary composite and its first member are starters"
    pool, pool_at, dec, runs = [], {}, [], []

    def pooled(s: str) -> int:
        key = tuple(ord(x) for x in s)
        if key not in pool_at:
            pool_at[key] = len(pool)
            pool.extend(key)
        return pool_at[key] << 8 | len(key)

    longest = 0
    for cp in range(MAX_CP):
        if not is_scalar(cp):
            w = 0xF00   # (never decoded from UTF-8: stands for itself)
        else:
            ch = chr(cp)
            w = U.combining(ch)
            for bit, form in ((8, "NFC"), (10, "NFKC")):
                if boundary_before(cp, form):
                    w |= 1 << bit
                    if U.normalize(form, ch) == ch:
                        w |= 2 << bit
            if is_hangul_syllable(cp):
                w |= 1 << 12
            else:
                nfd, nfkd = U.normalize("NFD", ch), U.normalize("NFKD", ch)
                longest = max(longest, len(nfkd))
                if nfd != ch or nfkd != ch:
                    dec.append((cp, pooled(nfd) if nfd != ch else 0, pooled(nfkd) if nfkd != ch else 0))
        if not runs or runs[-1][1] != w:
            runs.append((cp, w))
    assert longest == 18 and len(dec) < (1 << 19) - 1 and len(pool) < (1 << 24)
    comp = sorted((a << 21 | b, c) for (a, b), c in pairs.items())
    return runs, dec, pool, comp


def c_array(ctype: str, name: str, values, per_line: int = 48) -> str:
    rows = [",".join(str(v) for v in values[i : i + per_line]) for i in range(0, len(values), per_line)]
    return f"static const {ctype} {name}[{len(values)}] = {{\n" + ",\n".join(rows) + "\n};\n"


def render_inc() -> str:
    runs, dec, pool, comp = build_tables()
    cps = [c for c, _, _ in dec]
    out = [
        "// kanpyo_amd/csrc/kgpu_normalize_data.inc -- GENERATED by tools/gen_normalize_tables.py from Python's unicodedata; do not edit.\n",
        "// The compact form (runs of equal property bits; decompositions by code point, as differences) is described there; kgpu_normalize_table.cpp,\n",
        "// the only file that includes this one, expands it into the tables of kgpu_normalize_core.h.\n",
        f'#define KGPU_NORM_UNIDATA "{U.unidata_version}"\n',
        c_array("uint32_t", "NORM_RUN_START", [c for c, _ in runs]),
        c_array("uint16_t", "NORM_RUN_BITS", [w for _, w in runs]),
        c_array("uint16_t", "NORM_DEC_STEP", [c - p for c, p in zip(cps, [0] + cps[:-1])]),   # a code point with a decomposition, minus the one before it
        c_array("uint32_t", "NORM_DEC_NFD", [d for _, d, _ in dec]),
        c_array("uint32_t", "NORM_DEC_NFKD", [k for _, _, k in dec]),
        c_array("uint32_t", "NORM_POOL_CP", pool),
        c_array("uint64_t", "NORM_COMP_KEY", [k for k, _ in comp], 24),
        c_array("uint32_t", "NORM_COMP_VAL", [v for _, v in comp]),
    ]
    steps = [c - p for c, p in zip(cps, [0] + cps[:-1])]
    assert max(steps) < 65536
    return "".join(out)


# ---- the fixture: inputs and what unicodedata makes of them -------------------------------------------------------------------------------
def fixture_cases():
    ka, dak = "ｶ", "ﾞ"   # half-width KA, half-width voiced sound mark
    cases = [
        ("ascii", "Hello, world 123"), ("japanese", "すもももももももものうち。東京都に住む"), ("empty", ""),
        ("mixed", "ﾊﾝｶｸｶﾀｶﾅﾃﾞｽ｡ＡＢＣ１２３㈱①ｶﾞｷﾞｸﾞ　東京"),
        ("ka_dakuten_at_16", "a" * 13 + ka + dak), ("ka_dakuten_across_16", "a" * 15 + ka + dak + "b"), ("ka_dakuten_bytes_across_16", "a" * 14 + ka + dak),
        ("ka_dakuten_at_64", "a" * 61 + ka + dak), ("ka_dakuten_across_64", "a" * 63 + ka + dak + "b"), ("ka_dakuten_bytes_across_64", "a" * 62 + ka + dak + "c"),
        ("e_dot_acute", "e\u0323\u0301"), ("e_acute_dot", "e\u0301\u0323"), ("u0344", "\u0344"), ("a_u0344", "a\u0344"), ("u0f73", "\u0f73"), ("ka_u0f73", "\u0f40\u0f73"),
        ("u1e9b_u0323", "\u1e9b\u0323"), ("ufdfa", "\ufdfa"), ("ufdfa_x3", "\ufdfa" * 3),
        ("hangul_l_v_t", "\u1100\u1161\u11a8"), ("hangul_lv_t", "\uac00\u11a8"), ("hangul_lvt_v", "\uac01\u1161"), ("hangul_l_v", "\u1100\u1161"),
        ("hangul_text", "\ud55c\uad6d\uc5b4 \ud14d\uc2a4\ud2b8"), ("hangul_lv_t_old", "\uac00\u11c3"), ("hangul_l_l_v", "\u1100\u1100\u1161"),
        ("ohm_angstrom", "\u2126\u212b"), ("cjk_compat", "\ufa10\U0002f800"), ("bengali", "\u09c7\u09be"), ("bengali_line", "\u0995\u09c7\u09be"),
        ("leading_mark", "\u0301abc"), ("leading_marks", "\u0301\u0323e"), ("mark_only", "\u3099"), ("ka_then_mark", "\u30ab\u3099"),
        ("halfwidth_mark_only", "\uff9e"), ("hiragana_ka_halfwidth_mark", "\u304b\uff9e"),
        ("fullwidth_run", "ＡＢＣＤＥＦＧＨＩＪＫＬＭＮＯＰＱＲＳＴＵＶＷＸＹＺ"), ("halfwidth_run", "ｱｲｳｴｵｶﾞｷﾞｸﾞｹﾞｺﾞﾊﾟﾋﾟﾌﾟﾍﾟﾎﾟ"),
        ("ligatures", "ﬁﬂﬃ ½ ² ™ ㍿ ㌔ ㍻"), ("ideographic_space", "東京　都"), ("circled", "①②③⑩⑳"), ("parenthesized", "㈱㈲㈹"),
        ("greek_tonos", "ά ά ΐ"), ("hebrew_marks", "אָּ"), ("arabic", "آ آ ﷲ"),
        ("supplementary", "\U0001d400\U0001d7ce \U0001f600 \U00011099\U000110ba"), ("kana_voiced", "が ぱ ゔ"),
        ("private_and_unassigned", "\U000f0000͸￾\U0010ffff"), ("nul_and_controls", "a\x00b\x1fc"),
        ("marks_63", "a" + "\u0301" * 63), ("marks_64", "a" + "\u0301" * 64), ("marks_65", "a" + "\u0301" * 65), ("marks_65_then_clean", "x" * 20 + "a" + "\u0316" * 65 + "ｶﾞ"),
        ("marks_mixed_64", "o" + "̣̖́̈" * 16), ("leading_marks_65", "\u0301" * 65), ("leading_marks_66", "\u0301" * 66),
        ("long_clean", "情報処理の基礎" * 12), ("long_dirty", "ﾃﾞｰﾀＤＡＴＡ①" * 12),
    ]
    for name, text in cases:
        yield name, text.encode("utf-8")
    for pad in (0, 1, 2, 3, 14, 15, 16, 17):
        yield f"pad_{pad}_ka_dakuten", b"x" * pad + (ka + dak).encode("utf-8") + b"y"
    for name, raw in (("truncated", b"ab\xe3\x81"), ("truncated_mid", b"\xe3\x81a"), ("overlong", b"\xc0\xaf"), ("overlong3", b"\xe0\x80\xaf"), ("surrogate", b"\xed\xa0\x80"),
                      ("ff", b"abc\xffdef"), ("stray_continuation", b"\x80"), ("beyond_10ffff", b"\xf4\x90\x80\x80"), ("dirty_then_invalid", "ｶﾞ".encode("utf-8") + b"\xfe")):
        yield "invalid_" + name, raw


def render_fixture() -> str:
    cases = []
    for name, raw in fixture_cases():
        c = {"name": name, "input": raw.hex()}
        for form in FORMS:
            out, status = normalize_line(raw, form)
            c[form.lower()] = out.hex()
            c["status_" + form.lower()] = status
        cases.append(c)
    head = json.dumps({"unidata_version": U.unidata_version, "max_segment": MAX_SEGMENT})[:-1]
    return head + ', "cases": [\n' + ",\n".join(json.dumps(c, ensure_ascii=True) for c in cases) + "\n]}\n"   # (one case per line)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "kanpyo_amd", "csrc"), help="directory of kgpu_normalize_data.inc")
    ap.add_argument("--fixture", action="store_true", help="also write tests/golden/fixture_normalize.json")
    args = ap.parse_args(argv)
    with open(os.path.join(args.out, "kgpu_normalize_data.inc"), "w", encoding="ascii", newline="\n") as f:
        f.write(render_inc())
    if args.fixture:
        with open(os.path.join(ROOT, "tests", "golden", "fixture_normalize.json"), "w", encoding="ascii", newline="\n") as f:
            f.write(render_fixture())
    pairs, _ = pairs_and_seconds()
    print(f"unicodedata {U.unidata_version}: {len(pairs)} composition pairs", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
