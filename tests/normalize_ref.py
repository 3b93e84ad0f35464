"""What the normalisation tests share: the generator's own reference (tools/gen_normalize_tables.py: boundaries, segments and the rules of
include/kanpyo_gpu.h over Python's unicodedata), the awkward pool the randomised strings are drawn from, and the library's host function."""
import ctypes as C
import functools
import importlib.util
import os
import unicodedata

import numpy as np

from conftest import ROOT, load_golden

FORMS = {"NFC": 1, "NFKC": 2}


def generator():
    spec = importlib.util.spec_from_file_location("gen_normalize_tables", os.path.join(ROOT, "tools", "gen_normalize_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = generator()
GEN.boundary_before = functools.lru_cache(maxsize=1 << 16)(GEN.boundary_before)   # (a pure function of its arguments: long lines ask for the same few code points)

# code points that decompose, compose, reorder or block: the fixture's cases as single code points, and their neighbours
AWKWARD = [ord(c) for c in "aeAo ｶﾞﾊﾟｱＡ１㈱①　東がカガ"] + [
    0x0300, 0x0301, 0x0308, 0x0316, 0x0323, 0x0327, 0x0344, 0x0345, 0x0F71, 0x0F72, 0x0F73, 0x0F40, 0x1E9B, 0x017F, 0xFDFA, 0x1100, 0x1161, 0x1175, 0x11A7, 0x11A8,
    0x11C2, 0x11C3, 0xAC00, 0xAC01, 0xD7A3, 0x2126, 0x212B, 0xFA10, 0x2F800, 0x09C7, 0x09BE, 0x09D7, 0x3099, 0x309A, 0xFF9E, 0xFF9F, 0x304B, 0x30AB, 0x0BC6, 0x0BBE,
    0x1B05, 0x1B35, 0x0CC6, 0x0CD5, 0x0CC2, 0x0DD9, 0x0DCF, 0x0DCA, 0x1025, 0x102E, 0x05D0, 0x05BC, 0x05B8, 0xFB2E, 0x0627, 0x0653, 0x0622, 0x1F71, 0x03B1, 0x0390,
    0x00C5, 0x00E9, 0x1EB9, 0x1D15E, 0x1D157, 0x1D165, 0x11099, 0x110BA, 0xFB01, 0x00BD, 0x2122, 0x33FF, 0x00A0, 0x2000, 0x0378, 0xE000, 0xFFFE, 0x10FFFF, 0x0041, 0x030A,
]


def scalar(rng) -> int:
    while True:
        cp = int(rng.integers(0, 0x110000))
        if not 0xD800 <= cp <= 0xDFFF:
            return cp


def random_strings(seed: int, count: int):
    """Seeded strings of 1 - 12 code points: 80 % from the awkward pool, 20 % from the whole range."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 13))
        out.append("".join(chr(AWKWARD[int(rng.integers(0, len(AWKWARD)))] if rng.random() < 0.8 else scalar(rng)) for _ in range(n)))
    return out


def versions_agree() -> bool:
    from kanpyo_amd import _lib

    return unicodedata.unidata_version == _lib.lib().kgpu_normalize_unicode_version().decode()


def host(data: bytes, form: str, capacity=None):
    """kgpu_normalize_host -> (rc, bytes written or b"", size reported, status)."""
    from kanpyo_amd import _lib

    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(data) * 11 if capacity is None else capacity
    out = np.full(cap + 8, 0xEE, dtype=np.uint8)
    got, st = C.c_uint64(0), C.c_uint8(0xEE)
    rc = _lib.lib().kgpu_normalize_host(FORMS[form], src.ctypes.data if src.size else None, src.size, out.ctypes.data, cap, C.byref(got), C.byref(st))
    assert (out[cap:] == 0xEE).all(), "the host function wrote past its capacity"
    if rc != 0:
        assert (out == 0xEE).all(), "a failed call wrote something"
        return rc, b"", int(got.value), int(st.value)
    return rc, out[: got.value].tobytes(), int(got.value), int(st.value)


def host_lines(lines, form: str):
    """The host function over a list of lines -> (packed text, offsets, status) as the batch calls return them."""
    outs, sts = [], []
    for ln in lines:
        rc, out, _, st = host(bytes(ln), form)
        assert rc == 0
        outs.append(out)
        sts.append(st)
    off = np.zeros(len(outs) + 1, dtype=np.uint64)
    if outs:
        off[1:] = np.cumsum([len(o) for o in outs])
    return np.frombuffer(b"".join(outs), dtype=np.uint8), off, np.array(sts, dtype=np.uint8)


def fixture_cases():
    g = load_golden("fixture_normalize.json")
    return g, [(c["name"], bytes.fromhex(c["input"]), {f: (bytes.fromhex(c[f.lower()]), c["status_" + f.lower()]) for f in FORMS}) for c in g["cases"]]


# ---- what the sweeps share (tests/test_gpu_normalize_sweep.py) -------------------------------------------------------------------------------------
def strict_utf8(data: bytes) -> bool:
    """Does Python's strict decoder accept the line?"""
    try:
        data.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@functools.lru_cache(maxsize=None)
def scalars() -> np.ndarray:
    """All 1 112 064 scalar values, ascending."""
    cps = np.arange(0x110000, dtype=np.uint32)
    return cps[(cps < 0xD800) | (cps > 0xDFFF)]


def utf8_len(cps: np.ndarray) -> np.ndarray:
    """Bytes of each code point's encoding."""
    return 1 + (cps >= 0x80).astype(np.int64) + (cps >= 0x800) + (cps >= 0x10000)


def pack_strings(strs, line_bytes: np.ndarray):
    """Lines that are Python strings, their byte lengths known -> (utf8, offsets) as pack_sentences gives them, with one encode for the batch."""
    utf8 = np.frombuffer("".join(strs).encode("utf-8"), dtype=np.uint8)
    offs = np.zeros(len(strs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(line_bytes)
    assert int(offs[-1]) == utf8.size
    return utf8, offs


def normalize_strings(strs, form: str):
    """unicodedata over every line -> (text[uint8], offsets[uint64 n + 1], bytes per line, code points per line, changed[bool]), without a bytes object per line."""
    outs = [unicodedata.normalize(form, s) for s in strs]
    joined = "".join(outs)
    chars = np.fromiter(map(len, outs), dtype=np.int64, count=len(outs))
    changed = np.fromiter((o != s for o, s in zip(outs, strs)), dtype=bool, count=len(outs))
    per_cp = utf8_len(np.frombuffer(joined.encode("utf-32-le"), dtype="<u4"))
    ends = np.concatenate([[0], np.cumsum(per_cp)])[np.cumsum(chars)]
    offs = np.concatenate([[0], ends]).astype(np.uint64)
    text = np.frombuffer(joined.encode("utf-8"), dtype=np.uint8)
    assert int(offs[-1]) == text.size
    return text, offs, np.diff(offs.astype(np.int64)), chars, changed


@functools.lru_cache(maxsize=None)
def boundary_table(form: str) -> np.ndarray:
    """The generator's boundary_before for every scalar value, in the order of scalars()."""
    cps = scalars()
    return np.fromiter((GEN.boundary_before(int(c), form) for c in cps), dtype=bool, count=cps.size)


def differing_lines(got_text, got_off, want_text, want_off) -> np.ndarray:
    """The lines whose bytes differ between two packed batches of equally many lines (a line of another length differs)."""
    g, w = got_off.astype(np.int64), want_off.astype(np.int64)
    glen, wlen = np.diff(g), np.diff(w)
    bad = glen != wlen
    if g[-1] > got_text.size or w[-1] > want_text.size or (glen < 0).any():
        return np.arange(len(wlen))   # (offsets that do not describe the text: nothing can be compared)
    same = np.repeat(~bad, wlen)
    idx = np.arange(int(w[0]), int(w[-1]))[same]
    shift = np.repeat(g[:-1] - w[:-1], wlen)[same]
    diff = idx[got_text[idx + shift] != want_text[idx]]
    bad[np.searchsorted(w, diff, side="right") - 1] = True
    return np.nonzero(bad)[0]
