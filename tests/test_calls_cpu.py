"""kanpyo_amd._calls alone, over entries written here (no device, no library call but kgpu_last_error): the one retry rule, the growth of the
block protocol's two capacities, the out= checks of the multi-device call, and the module paths the moved names are still imported from."""
import importlib

import numpy as np
import pytest

from kanpyo_amd import _calls, _lib

CAPACITY = _lib.KGPU_ERR_CAPACITY


class NoLibrary:
    """All _calls needs of the library when an entry fails: the text of the error."""

    @staticmethod
    def kgpu_last_error():
        return b"said the entry"


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: NoLibrary)


def _sizes(total, n):
    return 8


def test_capacity_without_a_larger_size_is_an_error_after_one_call():
    """An entry that answers "capacity" and asks for no more than it was given is never called again, whoever owns the arrays."""
    utf8, offs = _calls.pack_sentences(["ab", "c"])
    for reported in (0, 7, 8):
        for kw in ({}, {"capacity": 8}, {"out": (np.empty(8, dtype=np.uint8), np.empty(3, dtype=np.uint64), np.empty(2, dtype=np.uint8))},
                   {"alloc": np.zeros, "slack": 64}):
            calls = []

            def entry(u, o, n, units, cap, uoff, st, got):
                calls.append(cap)
                got._obj.value = reported
                return CAPACITY

            with pytest.raises(_lib.KgpuError) as err:
                _calls.batch_call(entry, utf8, offs, np.uint8, _sizes, ("text[uint8]", "text_offsets"), **kw)
            assert err.value.code == CAPACITY and "said the entry" in str(err.value) and calls == [8]
    for got_v, n_v in ((0, 0), (10, 4), (9, 3)):   # capacities (10, 5): 10 units and 4 lines fit
        calls = []

        def entry(src, length, units, cap, uoff, ocap, st, n, got):
            calls.append((cap, ocap))
            n._obj.value, got._obj.value = n_v, got_v
            return CAPACITY

        with pytest.raises(_lib.KgpuError) as err:
            _calls.block_call(entry, b"a\nb\n", np.int32, lambda size: (10, 5))
        assert err.value.code == CAPACITY and calls == [(10, 5)]
    assert _calls.grown(0, (4,), (9,)) is None                     # (a call that succeeded is not repeated, whatever it reports)
    assert _calls.grown(CAPACITY, (4, 4), (9, 2), 1) == (10, 4)
    with pytest.raises(_lib.KgpuError):
        _calls.grown(_lib.KGPU_ERR_HIP, (4,), (9,))


def test_an_error_other_than_capacity_is_never_retried():
    utf8, offs = _calls.pack_sentences(["ab"])
    calls = []

    def entry(u, o, n, units, cap, uoff, st, got):
        calls.append(cap)
        got._obj.value = cap + 100
        return _lib.KGPU_ERR_INVALID_ARG

    with pytest.raises(_lib.KgpuError) as err:
        _calls.batch_call(entry, utf8, offs, np.uint8, _sizes, ("text[uint8]", "text_offsets"))
    assert err.value.code == _lib.KGPU_ERR_INVALID_ARG and calls == [8]


def test_block_capacities_only_grow():
    """Whatever an entry reports from call to call, neither capacity of the next call is below the last one's."""
    script = [(CAPACITY, 50, 2), (CAPACITY, 20, 30), (CAPACITY, 60, 1), (0, 3, 2)]   # (rc, units reported, lines reported) per call
    calls = []

    def entry(src, length, units, cap, uoff, ocap, st, n, got):
        rc, got_v, n_v = script[len(calls)]
        calls.append((cap, ocap))
        n._obj.value, got._obj.value = n_v, got_v
        return rc

    units, uoff, status = _calls.block_call(entry, np.frombuffer(b"a\nb\n", dtype=np.uint8), np.int32, lambda size: (size + 6, size + 1))
    assert calls == [(10, 5), (50, 5), (50, 31), (60, 31)]
    assert units.dtype == np.int32 and len(units) == 3 and len(uoff) == 3 and len(status) == 2


def test_the_multi_call_checks_out_like_the_others(monkeypatch):
    from kanpyo_amd.tokenizer import TOKEN8_DTYPE, TOKEN_DTYPE, tokenize_packed_multi

    class Tok:
        handle = None

    called = []

    class Entries(NoLibrary):
        kgpu_tokenize_batch_multi = kgpu_tokenize_batch_multi_compact = staticmethod(lambda *a: called.append(a))

    monkeypatch.setattr(_lib, "lib", lambda: Entries)
    utf8, offs = _calls.pack_sentences(["ab", "c"])
    for compact, dtype, other in ((False, TOKEN_DTYPE, TOKEN8_DTYPE), (True, TOKEN8_DTYPE, TOKEN_DTYPE)):
        good = (np.empty(9, dtype=dtype), np.empty(3, dtype=np.uint64), np.empty(2, dtype=np.uint8))
        for bad in ((np.empty(9, dtype=other), good[1], good[2]), (good[0], np.empty(2, dtype=np.uint64), good[2]), (good[0], good[1], np.empty(1, dtype=np.uint8)),
                    (good[0], good[1].astype(np.int64), good[2])):
            with pytest.raises(ValueError) as err:
                tokenize_packed_multi([Tok(), Tok()], utf8, offs, out=bad, compact=compact)
            assert not called and str(err.value) == f"out=(tokens[{'TOKEN8_DTYPE' if compact else 'TOKEN_DTYPE'}], tok_offsets[uint64 >= n+1], status[uint8 >= n])"


def test_packed_input():
    u, o, n, total = _calls.packed_input(list(b"abcdef"), [2, 4, 6])
    assert u.dtype == np.uint8 and o.dtype == np.uint64 and (n, total) == (2, 4)
    assert _calls.packed_input(np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))[2:] == (0, 0)
    with pytest.raises(ValueError, match=r"^offsets needs n\+1 entries$"):
        _calls.packed_input(u, [])
    a = np.arange(12, dtype=np.uint8)
    assert _calls.packed_input(a, o)[0] is a and _calls.packed_input(a[::2], o)[0].flags.c_contiguous
    assert _calls.block_bytes(a) is a and _calls.block_bytes(bytearray(b"xy")).tolist() == [120, 121] and _calls.ptr(a[:0]) is None


OLD_PATHS = {
    "kanpyo_amd": ["Token", "TokenClass", "Dict", "Tokenizer", "TOKEN_DTYPE", "Vocab", "_lib", "synth"],
    "kanpyo_amd.tokenizer": ["Tokenizer", "Words", "WordCounts", "TOKEN_DTYPE", "TOKEN8_DTYPE", "pack_sentences", "split_lines", "pinned_empty", "words_spec",
                             "tokenize_packed_multi", "concurrent_callers", "merge_shards", "merge_bench"],
    "kanpyo_amd.vocab": ["Vocab"],
    "kanpyo_amd.device": ["DeviceContext", "expand_tokens", "PROFILE_OFF", "PROFILE_EVENTS", "PROFILE_WORK", "PROFILE_SAMPLED", "PROFILE_NO_T", "STAGE_ALL",
                          "STAGE_LATTICE", "STAGE_GATHER", "STAGE_VITERBI"],
    "kanpyo_amd.cli": ["main", "parse_args", "first_line", "default_dict_path", "tokenize", "wakati", "count", "encode", "graphviz", "BLOCK_BYTES",
                       "PANIC_STATUS", "WHITE_SPACE"],
}


@pytest.mark.parametrize("module", list(OLD_PATHS))
def test_every_name_is_importable_from_where_it_was(module):
    import kanpyo_amd.synth  # noqa: F401  (`from kanpyo_amd import synth` is how the tests and the tools get it)

    m = importlib.import_module(module)
    missing = [name for name in OLD_PATHS[module] if not hasattr(m, name)]
    assert not missing
    from kanpyo_amd import device, tokenizer

    assert tokenizer.TOKEN_DTYPE is _calls.TOKEN_DTYPE is device.TOKEN_DTYPE and tokenizer.TOKEN8_DTYPE is _calls.TOKEN8_DTYPE   # defined once
    assert tokenizer.pack_sentences is _calls.pack_sentences and tokenizer.pinned_empty is _calls.pinned_empty


def test_calls_imports_neither_the_tokenizer_nor_torch():
    """Beside the standard library: numpy and _lib, so the module loads before (and without) every other module of the package."""
    import ast

    with open(_calls.__file__, encoding="utf-8") as f:
        tree = ast.parse(f.read())
    seen = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            seen.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            seen.update("." * node.level + (node.module or "") + ":" + a.name for a in node.names if node.level) if node.level else seen.add(node.module)
    assert seen == {"__future__", "ctypes", "weakref", "typing", "numpy", ".:_lib"}
