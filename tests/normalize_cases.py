"""What the tests of the text normaliser and of the alignment behind it share: the clean and dirty pieces and the lines mixed from them, the dictionary
whose keys are what half-width and full-width text normalises to (the `env` fixture of tests/test_gpu_normalize.py and tests/test_gpu_align.py), the
skip mark for a Python whose Unicode tables are not the committed ones, and the stub that stands where the library stands in the binding tests
(tests/test_normalize_cpu.py, tests/test_align_cpu.py).  Imports without a device and without the built library; same_unicode() loads it."""
import ctypes as C
import functools
import unicodedata

import numpy as np
import pytest

import normalize_ref as N
from conftest import fixture_dict_parts
from kanpyo_amd import _lib

KA, DAKUTEN = "ｶ", "ﾞ"
DIRTY = ["ﾊﾝｶｸｶﾀｶﾅ", "ＡＢＣ１２３", "㈱①", "ｶﾞｷﾞｸﾞ", "　", "e\u0301", "\u1100\u1161\u11a8", "\ufdfa", "a\u0323\u0301", "\u2126\u212b", "\ufa10", "ﾊﾟ"]
CLEAN = ["東京", "すもも", "abc", " ", "テスト", "。", "辞書", "xyz 123", "形態素"]


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """The reference's test dictionary with a few more keys -- among them what half-width and full-width text normalises to -- and display tables."""
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = fixture_dict_parts()
    keys = sorted(["テスト", "辞書", "形態素", "ハンカク", "ABC", "(株)", "ガ", "東京", "123"], key=lambda s: s.encode())
    p["sorted_keywords"] = keys
    p["morphs"] = [[i % 3, i % 3, 1000 + 10 * i] for i in range(len(keys))]
    e = Env()
    e.dict = Dict.from_parts(**p)
    e.known = MorphFeatureTable.from_features([["名詞"]] * len(keys))
    e.unk = MorphFeatureTable.from_features([["未知"]] * len(p["unk_morphs"]))
    e.tok = Tokenizer(e.dict)
    e.tok.set_features(e.known, e.unk)
    e.keys = keys
    return e


def mixed_lines(n, seed, max_bytes=200):
    """n lines of clean and dirty pieces, 0 .. max_bytes bytes each (every fourth one clean, some empty)."""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        want = int(rng.integers(0, max_bytes + 1))
        pool = CLEAN if i % 4 == 0 else CLEAN + DIRTY
        s = b""
        while True:
            piece = pool[int(rng.integers(0, len(pool)))].encode()
            if len(s) + len(piece) > want:
                break
            s += piece
        lines.append(s)
    return lines


SENTENCES = ["ﾊﾝｶｸＡＢＣ㈱", "テスト辞書", "", "形態素ｶﾞ東京１２３", "あいうえお", "ﾃｽﾄ辞書ｶﾞ", "ＡＢＣ" * 30, "漢字ﾊﾝｶｸ", "a" + "\u0301" * 65, "東京"] * 7


def same_unicode():
    """the skipif mark of a test that compares with Python's unicodedata"""
    return pytest.mark.skipif(not N.versions_agree(), reason=f"Python's unicodedata is {unicodedata.unidata_version}, the committed tables are "
                              f"{_lib.lib().kgpu_normalize_unicode_version().decode()}")


# ---- the binding over a stub library ------------------------------------------------------------------------------------------------------------------
def view(addr, dtype, count):
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_uint8 * max(count * dt.itemsize, 1)).from_address(addr), dtype=dt)[:count]


class StubLib:
    """Stands where _lib.lib() stands: logs the entry points reached.  A normalise entry upper-cases ASCII, leaves the offsets and marks line 1 with status 4; every other
    batch / block entry writes one unit per line and status 0."""

    def __init__(self):
        self.log, self.seen = [], []
        self._next = 0x1000
        for kind in ("dict", "words", "counts", "vocab"):
            setattr(self, f"kgpu_{kind}_create", functools.partial(self._create, kind))
            setattr(self, f"kgpu_{kind}_destroy", lambda h: None)

    def kgpu_last_error(self):
        return b"stub"

    def _create(self, kind, *args):
        self._next += 0x10
        args[-1]._obj.value = self._next
        return 0

    def kgpu_dict_get_info(self, h, ref):
        ref._obj.device = 0
        return 0

    def kgpu_normalize_batch(self, h, form, u, o, n, text, cap, toff, st, got):
        self.log.append(("normalize_batch", form))
        off = view(o, np.uint64, n + 1)
        total = int(off[n] - off[0])
        got._obj.value = total
        if total > cap:
            return _lib.KGPU_ERR_CAPACITY
        view(text, np.uint8, total)[:] = np.frombuffer(view(u, np.uint8, int(off[n]))[int(off[0]):].tobytes().upper(), dtype=np.uint8)
        view(toff, np.uint64, n + 1)[:] = off - off[0]
        view(st, np.uint8, n)[:] = [4 if i == 1 else 0 for i in range(n)]
        return 0

    def kgpu_normalize_text(self, h, form, src, length, text, cap, toff, ocap, st, n_ref, got):
        self.log.append(("normalize_text", form))
        lines = view(src, np.uint8, length).tobytes().upper().split(b"\n")[:-1]
        n_ref._obj.value, got._obj.value = len(lines), sum(map(len, lines))
        if got._obj.value > cap or len(lines) + 1 > ocap:
            return _lib.KGPU_ERR_CAPACITY
        view(text, np.uint8, got._obj.value)[:] = np.frombuffer(b"".join(lines), dtype=np.uint8)
        view(toff, np.uint64, len(lines) + 1)[:] = np.cumsum([0] + [len(x) for x in lines])
        view(st, np.uint8, len(lines))[:] = [4 if i == 1 else 0 for i in range(len(lines))]
        return 0

    def _batch(self, name, itemsize, h, u, o, n, units, cap, uoff, st, got):
        off = view(o, np.uint64, n + 1)
        self.log.append(name)
        self.seen.append(view(u, np.uint8, int(off[n])).tobytes() if n and int(off[n]) else b"")
        got._obj.value = n
        if n > cap:
            return _lib.KGPU_ERR_CAPACITY
        view(units, np.uint8, n * itemsize)[:] = 0
        view(uoff, np.uint64, n + 1)[:] = np.arange(n + 1)
        view(st, np.uint8, n)[:] = [1 if i == 2 else 0 for i in range(n)]
        return 0

    def _block(self, name, itemsize, h, src, length, units, cap, uoff, ocap, st, n_ref, got):
        self.log.append(name)
        n = view(src, np.uint8, length).tobytes().count(b"\n")
        n_ref._obj.value, got._obj.value = n, n
        if n > cap or n + 1 > ocap:
            return _lib.KGPU_ERR_CAPACITY
        view(uoff, np.uint64, n + 1)[:] = np.arange(n + 1)
        view(st, np.uint8, n)[:] = 0
        return 0

    def kgpu_count_batch(self, h, u, o, n, st):
        self.log.append("count_batch")
        off = view(o, np.uint64, n + 1)
        self.seen.append(view(u, np.uint8, int(off[n])).tobytes())
        view(st, np.uint8, n)[:] = 0
        return 0

    def kgpu_count_text(self, h, src, length, st, cap, n_ref):
        self.log.append("count_text")
        n_ref._obj.value = view(src, np.uint8, length).tobytes().count(b"\n")
        return 0


for _name, _size in (("tokenize_batch", 24), ("tokenize_batch_lines", 1), ("tokenize_batch_words", 1), ("encode_batch", 4)):
    setattr(StubLib, "kgpu_" + _name, functools.partialmethod(StubLib._batch, _name, _size))
for _name, _size in (("tokenize_text_lines", 1), ("tokenize_text_words", 1), ("encode_text", 4)):
    setattr(StubLib, "kgpu_" + _name, functools.partialmethod(StubLib._block, _name, _size))
