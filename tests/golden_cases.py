"""What the CPU tests of the record consumers (words, counts, vocabulary ids, table keys) share: the record layout, the fixture dictionary's display
rows, the hand-derived records of tests/golden/fixture_tokens.json packed as a call takes them, the 20 000-record synthetic dictionary with its
feature tables, and the kgpu_debug_vocab_table hook.  Imports without a device; only vocab_table loads the library, when it is called."""
import ctypes as C

import numpy as np
import pytest

from conftest import fixture_dict_parts, load_golden
from kanpyo_amd.dictfile import MorphFeatureTable

TOKEN_DTYPE = np.dtype([("id", "<i4"), ("cls", "<u4"), ("position", "<u4"), ("start", "<u4"), ("end", "<u4"), ("byte_len", "<u4")])


def fixture_tables():
    """The display rows of tests/test_gpu_lines.py::test_fixture_dictionary_hand_derived."""
    p = fixture_dict_parts()
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, len(p["unk_morphs"]) + 1)])
    return p, known, unk


def golden_records(sentences):
    """The hand-derived tokens of tests/golden/fixture_tokens.json for these sentences, packed -> (utf8 bytes, offsets, tokens, tok_offsets)."""
    tokens_of = {c["input"]: c["tokens"] for c in load_golden("fixture_tokens.json")["cases"]}
    raw, offs, recs, toff = b"", [0], [], [0]
    for s in sentences:
        raw += s.encode()
        offs.append(len(raw))
        for tid, cls, pos, start, end, surface in tokens_of[s]:
            recs.append((tid, cls, pos, start, end, 0 if cls == 0 else len(surface.encode())))
        toff.append(len(recs))
    tokens = np.zeros(len(recs), dtype=TOKEN_DTYPE)
    for i, r in enumerate(recs):
        tokens[i] = r
    return raw, np.array(offs, dtype=np.uint64), tokens, np.array(toff, dtype=np.uint64)


@pytest.fixture(scope="module")
def synth20k():
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    return sd, known, unk, len(known.morph_features), len(unk.morph_features), synth.record_surfaces(sd)


def vocab_table(sd_dict, known, unk, nk, nu, kw, words, unk_id, flags=0, bos=0, eos=0):
    """kgpu_debug_vocab_table -> (rc, row_id int32[nk + nu], slots uint64[n, 2], arena bytes, rows_resolved)."""
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import pack_sentences, words_spec

    L = _lib.lib()
    spec, keep = words_spec(**kw)
    kb = np.frombuffer(known.encode(), dtype=np.uint8)
    ub = np.frombuffer(unk.encode(), dtype=np.uint8)
    ib = np.frombuffer(sd_dict.index_dict, dtype=np.uint8)
    packed, woff = pack_sentences(words)
    packed = np.ascontiguousarray(packed)
    opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), flags, unk_id, bos, eos)
    row_id = np.full(nk + nu, 0x5A5A5A5A, dtype=np.int32)
    ns, al, rr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    args = (kb.ctypes.data, kb.size, ub.ctypes.data, ub.size, ib.ctypes.data, ib.size, nk, nu, C.byref(spec), packed.ctypes.data if packed.size else None,
            woff.ctypes.data, len(words), C.byref(opts), row_id.ctypes.data)
    rc = L.kgpu_debug_vocab_table(*args, None, 0, C.byref(ns), None, 0, C.byref(al), C.byref(rr))
    if rc != _lib.KGPU_ERR_CAPACITY:
        return rc, row_id, None, None, int(rr.value)
    slots = np.zeros((int(ns.value), 2), dtype=np.uint64)
    arena = np.zeros(max(int(al.value), 1), dtype=np.uint8)
    rc = L.kgpu_debug_vocab_table(*args, slots.ctypes.data, len(slots), C.byref(ns), arena.ctypes.data, int(al.value), C.byref(al), C.byref(rr))
    del keep
    return rc, row_id, slots, arena.tobytes()[: int(al.value)], int(rr.value)
