"""The Python binding above the C ABI, characterised against a fake library (no device): what each wrapper hands to its entry point -- first
capacity, retry with the reported size, caller-owned out= arrays, the n = 0 call -- what it returns, the life cycle of the five handle classes,
and the command-line flows of `tokenize`, `wakati`, `count` and `encode` over stub objects.  Nothing here depends on how the wrappers are
written: the file describes what they do, and holds for any rewrite that leaves that alone."""
import ctypes as C
import functools
import gc
import io
from collections import Counter

import numpy as np
import pytest

from kanpyo_amd import _lib
from kanpyo_amd.tokenizer import TOKEN8_DTYPE, TOKEN_DTYPE, pack_sentences, split_lines, tokenize_packed_multi

CAPACITY = _lib.KGPU_ERR_CAPACITY
SENTENCES = ["すもも", "", "もも"]


def _view(addr, dtype, count):
    """The caller's memory at a raw address, as the library sees it."""
    dt = np.dtype(dtype)
    if count == 0:
        return np.empty(0, dtype=dt)
    return np.frombuffer((C.c_uint8 * (count * dt.itemsize)).from_address(addr), dtype=dt)


class FakeLib:
    """Stands where _lib.lib() stands.  A batch entry reports `need` units (default: two per sentence) and fills units, offsets and status through
    the addresses it was given, or answers KGPU_ERR_CAPACITY and writes nothing; a block entry does the same for `lines` lines."""

    def __init__(self):
        self.calls = []      # one dict per batch / block / count call
        self.events = []     # ("create" | "destroy", kind, handle)
        self.need = None
        self.lines = 3
        self.extra = None    # graphviz: (dpi, full_state)
        self.pinned = {}
        self._next = 0x1000
        for kind in ("dict", "words", "counts", "vocab", "ctx"):
            setattr(self, f"kgpu_{kind}_create", functools.partial(self._create, kind))
            setattr(self, f"kgpu_{kind}_destroy", functools.partial(self._destroy, kind))

    def kgpu_last_error(self):
        return b"the fake library says no"

    def _create(self, kind, *args):
        self._next += 0x10
        args[-1]._obj.value = self._next
        self.events.append(("create", kind, self._next))
        return 0

    def _destroy(self, kind, h):
        self.events.append(("destroy", kind, getattr(h, "value", h)))

    def destroyed(self, kind):
        return [h for what, k, h in self.events if what == "destroy" and k == kind]

    def kgpu_dict_get_info(self, h, ref):
        ref._obj.device, ref._obj.n_morphs = 0, 7
        return 0

    def kgpu_counts_get_info(self, h, ref):
        ref._obj.tokens_counted = 11
        return 0

    def kgpu_vocab_get_info(self, h, ref):
        ref._obj.n_words = 3
        return 0

    def kgpu_dict_set_features(self, *args):
        return 0

    def kgpu_host_alloc(self, nbytes):
        buf = (C.c_uint8 * nbytes)()
        self.pinned[C.addressof(buf)] = buf
        return C.addressof(buf)

    def kgpu_host_free(self, p):
        del self.pinned[p]

    # ---- batch entries --------------------------------------------------------------------------------------------------------------------
    def _batch(self, name, itemsize, u, o, n, units, cap, uoff, st, got, **more):
        need = 2 * n if self.need is None else self.need
        self.calls.append(dict(name=name, cap=cap, n=n, utf8=u, offsets=o, units=units, uoff=uoff, status=st, status_in=_view(st, np.uint8, n).copy(), **more))
        got._obj.value = need
        if need > cap:
            return CAPACITY
        _view(units, np.uint8, need * itemsize)[:] = 0xAB
        _view(uoff, np.uint64, n + 1)[:] = self.offsets(n, need)
        _view(st, np.uint8, n)[:] = self.status(n)
        return 0

    @staticmethod
    def offsets(n, need):
        return (np.arange(n + 1, dtype=np.uint64) * np.uint64(need)) // np.uint64(max(n, 1))

    @staticmethod
    def status(n):
        return (np.arange(n) & 1).astype(np.uint8)

    def kgpu_tokenize_batch(self, h, *a):
        return self._batch("tokenize_batch", 24, *a)

    def kgpu_tokenize_batch_lines(self, h, *a):
        return self._batch("tokenize_batch_lines", 1, *a)

    def kgpu_tokenize_batch_words(self, h, *a):
        return self._batch("tokenize_batch_words", 1, *a)

    def kgpu_encode_batch(self, h, *a):
        return self._batch("encode_batch", 4, *a)

    def kgpu_graphviz_batch(self, h, u, o, n, dpi, full_state, *rest):
        self.extra = (dpi, full_state)
        return self._batch("graphviz_batch", 1, u, o, n, *rest)

    def kgpu_tokenize_batch_multi(self, handles, G, *a):
        return self._batch("tokenize_batch_multi", 24, *a, G=G)

    def kgpu_tokenize_batch_multi_compact(self, handles, G, u, o, n, units, cap, first, uoff, st, got):
        return self._batch("tokenize_batch_multi_compact", 8, u, o, n, units, cap, uoff, st, got, G=G, first=first)

    def kgpu_count_batch(self, h, u, o, n, st):
        self.calls.append(dict(name="count_batch", n=n, utf8=u, status_in=_view(st, np.uint8, n).copy()))
        _view(st, np.uint8, n)[:] = self.status(n)
        return 0

    # ---- raw-block entries ----------------------------------------------------------------------------------------------------------------
    def _block(self, name, itemsize, h, src, length, units, cap, uoff, ocap, st, n_ref, got):
        k = self.lines
        need = 2 * k if self.need is None else self.need
        self.calls.append(dict(name=name, cap=cap, ocap=ocap, src=src, len=length, text=_view(src, np.uint8, length).tobytes(), status_in=_view(st, np.uint8, ocap).copy()))
        n_ref._obj.value, got._obj.value = k, need
        if need > cap or k + 1 > ocap:
            return CAPACITY
        _view(units, np.uint8, need * itemsize)[:] = 0xAB
        _view(uoff, np.uint64, k + 1)[:] = self.offsets(k, need)
        _view(st, np.uint8, k)[:] = self.status(k)
        return 0

    def kgpu_tokenize_text_lines(self, *a):
        return self._block("tokenize_text_lines", 1, *a)

    def kgpu_tokenize_text_words(self, *a):
        return self._block("tokenize_text_words", 1, *a)

    def kgpu_encode_text(self, *a):
        return self._block("encode_text", 4, *a)

    def kgpu_count_text(self, h, src, length, st, cap, n_ref):
        k = self.lines
        self.calls.append(dict(name="count_text", cap=cap, src=src, len=length, text=_view(src, np.uint8, length).tobytes()))
        n_ref._obj.value = k
        if k > cap:
            return CAPACITY
        _view(st, np.uint8, k)[:] = self.status(k)
        return 0


class Env:
    pass


@pytest.fixture
def env(fixture_dict, monkeypatch):
    """A Tokenizer, a Words, a WordCounts and a Vocab (with a BOS id: one extra id per sentence) over the fake library.  The fixture dictionary
    is built first, by the real host library; every handle is closed before the patch is undone, so that no __del__ meets the real one."""
    from kanpyo_amd import Tokenizer

    e = Env()
    e.lib = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: e.lib)
    e.tok = Tokenizer(fixture_dict)
    e.words = e.tok.words()
    e.counts = e.words.counter()
    e.vocab = e.words.vocabulary(["<unk>", "<s>", "もも"], unk_id=0, bos_id=1)
    e.made = [e.vocab, e.counts, e.words, e.tok]
    yield e
    for obj in e.made:
        obj.close()
    gc.collect()


def _compact(e, utf8, offsets, **kw):
    units, first, uoff, status = tokenize_packed_multi([e.tok, e.tok], utf8, offsets, compact=True, **kw)
    assert first.dtype == np.uint32 and first.shape == (len(status), 2) and e.lib.calls[-1]["first"] == first.ctypes.data
    return units, uoff, status


# name -> (the call, unit dtype, first capacity of (total bytes, n), slack added to a reported size, takes out=, validates out=)
BATCH = {
    "tokenize_packed": (lambda e: e.tok.tokenize_packed, TOKEN_DTYPE, lambda t, n: t // 2 + n + 64, 64, True, True),
    "tokenize_lines_packed": (lambda e: e.tok.tokenize_lines_packed, np.uint8, lambda t, n: t * 16 + 8 * n + 64, 0, True, True),
    "graphviz_packed": (lambda e: e.tok.graphviz_packed, np.uint8, lambda t, n: t * 512 + 1024 * n + 64, 0, False, False),
    "render_packed": (lambda e: e.words.render_packed, np.uint8, lambda t, n: t * 2 + n + 64, 0, True, True),
    "encode_packed": (lambda e: e.vocab.encode_packed, np.int32, lambda t, n: t // 2 + n * 2 + 64, 0, True, True),
    # (before the wrappers shared one body the multi call handed out= on unchecked: its dtype and length checks are tested with that body,
    # in test_calls_cpu.py, so that this file describes both)
    "multi": (lambda e: functools.partial(tokenize_packed_multi, [e.tok, e.tok]), TOKEN_DTYPE, lambda t, n: t // 2 + n + 64, 64, True, False),
    "multi_compact": (lambda e: functools.partial(_compact, e), TOKEN8_DTYPE, lambda t, n: t // 2 + n + 64, 64, True, False),
}
WITH_OUT = [k for k, v in BATCH.items() if v[4]]
CHECKS_OUT = [k for k, v in BATCH.items() if v[5]]


def _out(dtype, cap, n, status_fill=7):
    return np.empty(cap, dtype=dtype), np.empty(n + 1, dtype=np.uint64), np.full(n, status_fill, dtype=np.uint8)


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_call_with_enough_room(env, name):
    make, dtype, first, _, _, _ = BATCH[name]
    utf8, offs = pack_sentences(SENTENCES)
    units, uoff, status = make(env)(utf8, offs)
    (call,) = env.lib.calls
    assert call["n"] == 3 and call["cap"] == first(utf8.size, 3) and call["utf8"] == utf8.ctypes.data and call["offsets"] == offs.ctypes.data
    assert not call["status_in"].any()
    assert units.dtype == np.dtype(dtype) and len(units) == 6 and uoff.dtype == np.uint64 and status.dtype == np.uint8
    assert np.array_equal(uoff, FakeLib.offsets(3, 6)) and np.array_equal(status, FakeLib.status(3))
    assert np.array_equal(units.view(np.uint8), np.full(6 * np.dtype(dtype).itemsize, 0xAB, dtype=np.uint8))


def test_graphviz_arguments_reach_the_entry(env):
    utf8, offs = pack_sentences(SENTENCES)
    env.tok.graphviz_packed(utf8, offs, dpi=96, full_state=True)
    assert env.lib.extra == (96, 1)
    env.tok.graphviz_packed(utf8, offs)
    assert env.lib.extra == (48, 0)


def test_pinned_results_come_from_the_library_allocator(env):
    utf8, offs = pack_sentences(SENTENCES)
    units, uoff, status = env.tok.tokenize_packed(utf8, offs, pinned=True)
    assert {units.ctypes.data, uoff.ctypes.data, status.ctypes.data} == set(env.lib.pinned)
    assert len(units) == 6 and len(uoff) == 4 and len(status) == 3
    del units, uoff, status
    gc.collect()
    assert not env.lib.pinned


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_call_with_too_little_room_asks_once_more(env, name):
    make, dtype, first, slack, _, _ = BATCH[name]
    utf8, offs = pack_sentences(SENTENCES)
    env.lib.need = first(utf8.size, 3) + 100
    units, uoff, status = make(env)(utf8, offs)
    assert [c["cap"] for c in env.lib.calls] == [first(utf8.size, 3), env.lib.need + slack]
    assert len(units) == env.lib.need and len(uoff) == 4 and len(status) == 3 and not env.lib.calls[1]["status_in"].any()


@pytest.mark.parametrize("name", WITH_OUT)
def test_out_arrays_are_used_as_they_are(env, name):
    make, dtype, _, _, _, _ = BATCH[name]
    utf8, offs = pack_sentences(SENTENCES)
    out = _out(dtype, 9, 3)
    units, uoff, status = make(env)(utf8, offs, out=out)
    (call,) = env.lib.calls
    assert (call["units"], call["uoff"], call["status"], call["cap"]) == (out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 9)
    assert not call["status_in"].any()                     # (the caller's 7s were cleared before the call)
    assert all(np.shares_memory(a, b) for a, b in zip((units, uoff, status), out)) and len(units) == 6 and len(uoff) == 4 and len(status) == 3
    # longer offsets / status arrays than needed are fine and come back cut to n + 1 and n
    big = (np.empty(9, dtype=dtype), np.empty(10, dtype=np.uint64), np.empty(10, dtype=np.uint8))
    units, uoff, status = make(env)(utf8, offs, out=big)
    assert len(units) == 6 and len(uoff) == 4 and len(status) == 3


@pytest.mark.parametrize("name", WITH_OUT)
def test_out_too_small_is_an_error_not_a_reallocation(env, name):
    make, dtype, _, _, _, _ = BATCH[name]
    utf8, offs = pack_sentences(SENTENCES)
    out = _out(dtype, 4, 3)
    with pytest.raises(_lib.KgpuError) as err:
        make(env)(utf8, offs, out=out)
    assert err.value.code == CAPACITY and "the fake library says no" in str(err.value)
    (call,) = env.lib.calls
    assert (call["units"], call["uoff"], call["status"], call["cap"]) == (out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 4)


@pytest.mark.parametrize("name", ["tokenize_packed", "multi", "multi_compact"])
def test_an_explicit_token_capacity_is_not_grown(env, name):
    utf8, offs = pack_sentences(SENTENCES)
    with pytest.raises(_lib.KgpuError) as err:
        BATCH[name][0](env)(utf8, offs, token_capacity=4)
    assert err.value.code == CAPACITY and [c["cap"] for c in env.lib.calls] == [4]
    units, _, _ = BATCH[name][0](env)(utf8, offs, token_capacity=6)
    assert len(units) == 6 and env.lib.calls[-1]["cap"] == 6


@pytest.mark.parametrize("name", CHECKS_OUT)
def test_out_of_the_wrong_kind_is_refused_before_any_call(env, name):
    make, dtype, _, _, _, _ = BATCH[name]
    utf8, offs = pack_sentences(SENTENCES)
    other = np.uint16 if np.dtype(dtype) != np.uint16 else np.uint8
    good = _out(dtype, 9, 3)
    for bad in ((np.empty(9, dtype=other), good[1], good[2]), (good[0], np.empty(4, dtype=np.int64), good[2]), (good[0], good[1], np.empty(3, dtype=np.int8)),
                (good[0], np.empty(3, dtype=np.uint64), good[2]), (good[0], good[1], np.empty(2, dtype=np.uint8))):
        with pytest.raises(ValueError, match=r"^out=\(\w+\[\w+\], \w+\[uint64 >= n\+1\], status\[uint8 >= n\]\)$"):
            make(env)(utf8, offs, out=bad)
    assert not env.lib.calls


def test_each_out_message_names_its_own_unit(env):
    utf8, offs = pack_sentences(SENTENCES)
    bad = (np.empty(9, dtype=np.uint16), np.empty(4, dtype=np.uint64), np.empty(3, dtype=np.uint8))
    for call, text in ((env.tok.tokenize_packed, "out=(tokens[TOKEN_DTYPE], tok_offsets[uint64 >= n+1], status[uint8 >= n])"),
                       (env.tok.tokenize_lines_packed, "out=(text[uint8], text_offsets[uint64 >= n+1], status[uint8 >= n])"),
                       (env.words.render_packed, "out=(text[uint8], text_offsets[uint64 >= n+1], status[uint8 >= n])"),
                       (env.vocab.encode_packed, "out=(ids[int32], id_offsets[uint64 >= n+1], status[uint8 >= n])")):
        with pytest.raises(ValueError) as err:
            call(utf8, offs, out=bad)
        assert str(err.value) == text


@pytest.mark.parametrize("name", list(BATCH) + ["add_packed"])
def test_offsets_without_an_entry_are_refused(env, name):
    call = env.counts.add_packed if name == "add_packed" else BATCH[name][0](env)
    with pytest.raises(ValueError, match=r"^offsets needs n\+1 entries$"):
        call(np.empty(0, dtype=np.uint8), np.empty(0, dtype=np.uint64))
    assert not env.lib.calls


@pytest.mark.parametrize("name", list(BATCH))
def test_no_sentences_is_one_call_without_text(env, name):
    make, dtype, first, _, _, _ = BATCH[name]
    units, uoff, status = make(env)(np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    (call,) = env.lib.calls
    assert call["n"] == 0 and call["utf8"] is None and call["cap"] == first(0, 0)
    assert units.dtype == np.dtype(dtype) and len(units) == 0 and uoff.tolist() == [0] and len(status) == 0


def test_inputs_of_other_types_are_converted(env):
    """Lists and arrays of another dtype are as good as uint8 / uint64 arrays; offsets need not start at 0 (the total is the span)."""
    units, uoff, status = env.tok.tokenize_lines_packed(list(b"abcdef"), [2, 4, 6])
    (call,) = env.lib.calls
    assert call["n"] == 2 and call["cap"] == 4 * 16 + 8 * 2 + 64 and len(units) == 4 and len(uoff) == 3 and len(status) == 2


def test_count_batch(env):
    utf8, offs = pack_sentences(SENTENCES)
    status = env.counts.add_packed(utf8, offs)
    (call,) = env.lib.calls
    assert call["n"] == 3 and call["utf8"] == utf8.ctypes.data and not call["status_in"].any() and np.array_equal(status, FakeLib.status(3))
    assert len(env.counts.add_packed(np.empty(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))) == 0
    assert env.lib.calls[-1]["n"] == 0 and env.lib.calls[-1]["utf8"] is None
    assert np.array_equal(env.counts.add(SENTENCES), FakeLib.status(3))


# ---- the raw-block calls -------------------------------------------------------------------------------------------------------------------
BLOCK = b"a b\n\nc d e\n" * 4   # 40 bytes
OCAP = len(BLOCK) // 16 + 1024
TEXT = {
    "tokenize_text_lines": (lambda e: e.tok.tokenize_text_lines, np.uint8, len(BLOCK) * 16 + 64),
    "render_text": (lambda e: e.words.render_text, np.uint8, len(BLOCK) * 2 + 64),
    "encode_text": (lambda e: e.vocab.encode_text, np.int32, len(BLOCK) // 2 + 64 + OCAP),   # (one BOS per possible line)
}


@pytest.mark.parametrize("form", [bytes, bytearray, memoryview, lambda b: np.frombuffer(b, dtype=np.uint8)])
@pytest.mark.parametrize("name", list(TEXT))
def test_text_call_with_enough_room(env, name, form):
    make, dtype, cap = TEXT[name]
    units, uoff, status = make(env)(form(BLOCK))
    (call,) = env.lib.calls
    assert (call["cap"], call["ocap"], call["len"]) == (cap, OCAP, len(BLOCK)) and not call["status_in"].any()
    assert call["text"] == BLOCK
    assert units.dtype == np.dtype(dtype) and len(units) == 6 and np.array_equal(uoff, FakeLib.offsets(3, 6)) and np.array_equal(status, FakeLib.status(3))


@pytest.mark.parametrize("name", list(TEXT))
@pytest.mark.parametrize("short", ["units", "offsets", "both"])
def test_text_call_grows_what_was_short_once(env, name, short):
    make, dtype, cap = TEXT[name]
    env.lib.need = cap + 10 if short in ("units", "both") else 2
    env.lib.lines = OCAP + 5 if short in ("offsets", "both") else 3
    units, uoff, status = make(env)(BLOCK)
    assert [(c["cap"], c["ocap"]) for c in env.lib.calls] == [(cap, OCAP), (max(cap, env.lib.need), max(OCAP, env.lib.lines + 1))]
    assert not env.lib.calls[1]["status_in"].any()
    assert len(units) == env.lib.need and len(uoff) == env.lib.lines + 1 and len(status) == env.lib.lines


@pytest.mark.parametrize("name", list(TEXT))
def test_text_call_over_the_empty_block(env, name):
    make, dtype, _ = TEXT[name]
    env.lib.lines = 0
    units, uoff, status = make(env)(b"")
    (call,) = env.lib.calls
    assert call["src"] is None and call["len"] == 0 and call["ocap"] == 1024
    assert units.dtype == np.dtype(dtype) and len(units) == 0 and uoff.tolist() == [0] and len(status) == 0


def test_count_text_with_more_lines_than_the_first_capacity(env):
    status = env.counts.add_text(BLOCK)
    assert [c["cap"] for c in env.lib.calls] == [OCAP] and env.lib.calls[0]["text"] == BLOCK and np.array_equal(status, FakeLib.status(3))
    env.lib.calls.clear()
    env.lib.lines = OCAP + 7
    status = env.counts.add_text(BLOCK)
    assert [c["cap"] for c in env.lib.calls] == [OCAP, OCAP + 7] and np.array_equal(status, FakeLib.status(OCAP + 7))
    env.lib.lines = 0
    assert len(env.counts.add_text(b"")) == 0 and env.lib.calls[-1]["src"] is None


# ---- handles -------------------------------------------------------------------------------------------------------------------------------
def test_every_handle_is_destroyed_exactly_once(env, fixture_dict):
    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import DeviceContext

    tok = Tokenizer(fixture_dict)
    words = tok.words()
    objs = {"ctx": DeviceContext(tok), "vocab": words.vocabulary(["a"], unk_id=0), "counts": words.counter(), "words": words, "dict": tok}
    del tok, words
    for kind in list(objs):
        obj = objs.pop(kind)
        h, before = obj._h.value, env.lib.destroyed(kind)
        assert ("create", kind, h) in env.lib.events and (kind == "ctx" or obj.handle is obj._h)
        obj.close()
        assert obj._h is None
        obj.close()
        del obj
        gc.collect()
        assert env.lib.destroyed(kind) == before + [h]
    # never closed: collected, destroyed once
    words = env.tok.words()
    h = words.handle.value
    del words
    gc.collect()
    assert env.lib.destroyed("words").count(h) == 1


def test_a_vocab_closes_its_context_first(env):
    from kanpyo_amd.device import DeviceContext

    env.vocab._ctx = DeviceContext(env.tok)
    hc, hv = env.vocab._ctx._h.value, env.vocab.handle.value
    env.vocab.close()
    assert [e for e in env.lib.events if e[0] == "destroy"] == [("destroy", "ctx", hc), ("destroy", "vocab", hv)]
    assert env.vocab._ctx is None
    env.vocab.close()
    assert len([e for e in env.lib.events if e[0] == "destroy"]) == 2


def test_closing_what_was_never_opened_is_silent(env):
    """A constructor that failed before the handle existed leaves an object without _h: close() and __del__ say nothing."""
    from kanpyo_amd import Tokenizer, Vocab
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import WordCounts, Words

    for cls in (Tokenizer, Words, WordCounts, Vocab, DeviceContext):
        obj = cls.__new__(cls)
        obj.close()
        del obj
    gc.collect()
    assert not [e for e in env.lib.events if e[0] == "destroy"]
    env.lib.kgpu_words_create = lambda *a: _lib.KGPU_ERR_INVALID_ARG
    with pytest.raises(_lib.KgpuError):
        env.tok.words()
    gc.collect()
    assert not env.lib.destroyed("words")


def test_info_reads(env):
    assert env.tok.info() == {"da_len": 0, "n_morphs": 7, "n_unk_morphs": 0, "conn_rows": 0, "conn_cols": 0, "device_bytes": 0, "device": 0}
    assert env.counts.info() == {"tokens_counted": 11, "overflow_tokens": 0, "sentences": 0, "table_slots": 0, "table_slots_used": 0, "key_bytes": 0,
                                 "key_bytes_used": 0}
    assert env.vocab.info() == {"n_words": 3, "table_slots": 0, "key_bytes": 0, "rows_resolved": 0}


# ---- the command line over stub objects ------------------------------------------------------------------------------------------------------
def _lines_of(utf8, offsets):
    raw, o = np.asarray(utf8, dtype=np.uint8).tobytes(), np.asarray(offsets).tolist()
    return [raw[o[i] : o[i + 1]] for i in range(len(o) - 1)]


def _valid(line):
    try:
        line.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _units(lines, per_line, dtype):
    """(units, offsets, status) of a stub call: per_line(line) units for a valid line, none and status 1 for a line that is not UTF-8."""
    parts = [per_line(ln) if _valid(ln) else [] for ln in lines]
    offs = np.zeros(len(lines) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    flat = [x for p in parts for x in p]
    return np.array(flat, dtype=dtype), offs, np.array([0 if _valid(ln) else 1 for ln in lines], dtype=np.uint8)


class StubTokenizer:
    log = None   # the calls of the run, set by the fixture

    def __init__(self, d):
        assert d == "the dictionary"
        self.log.append("open")

    def set_features(self, known, unk):
        assert (known, unk) == ("known table", "unk table")
        self.log.append("features")

    def tokenize_lines_packed(self, utf8, offsets):
        self.log.append("packed")
        return _units(_lines_of(utf8, offsets), lambda ln: list(ln + b"\tX\nEOS\n"), np.uint8)

    def tokenize_text_lines(self, block):
        self.log.append("text")
        return _units(_lines_of(*split_lines(block)), lambda ln: list(ln + b"\tX\nEOS\n"), np.uint8)

    def words(self, field=None, drop=(), keep=(), separator=" "):
        self.log.append(("words", field, list(drop), list(keep), separator))
        return StubWords(self.log)


class StubWords:
    def __init__(self, log):
        self.log = log

    def render_packed(self, utf8, offsets):
        self.log.append("packed")
        return _units(_lines_of(utf8, offsets), lambda ln: list(ln + b"\n"), np.uint8)

    def render_text(self, block):
        self.log.append("text")
        return _units(_lines_of(*split_lines(block)), lambda ln: list(ln + b"\n"), np.uint8)

    def counter(self):
        return StubCounts(self.log)


class StubCounts:
    def __init__(self, log):
        self.log, self.seen = log, Counter()

    def _add(self, utf8, offsets):
        lines = _lines_of(utf8, offsets)
        self.seen.update(w for ln in lines if _valid(ln) for w in ln.split())
        return np.array([0 if _valid(ln) else 1 for ln in lines], dtype=np.uint8)

    def add_packed(self, utf8, offsets):
        self.log.append("packed")
        return self._add(utf8, offsets)

    def add_text(self, block):
        self.log.append("text")
        return self._add(*split_lines(block))

    def most_common(self, n=None):
        return sorted(self.seen.items(), key=lambda kv: (-kv[1], kv[0]))[:n]


class StubVocab:
    def __init__(self, log):
        self.log = log

    def encode_packed(self, utf8, offsets):
        self.log.append("packed")
        return _units(_lines_of(utf8, offsets), lambda ln: [len(w) for w in ln.split()], np.int32)

    def encode_text(self, block):
        self.log.append("text")
        return _units(_lines_of(*split_lines(block)), lambda ln: [len(w) for w in ln.split()], np.int32)


class StubDictFile:
    dict, morph_feature_table, unk_feature_table = "the dictionary", "known table", "unk table"


@pytest.fixture
def cli_env(monkeypatch, tmp_path):
    """kanpyo_amd.cli with the dictionary file, the Tokenizer and the Vocab factory replaced; .run(argv, stdin bytes) -> (status, stdout bytes)."""
    from kanpyo_amd import cli, dictfile, tokenizer, vocab

    e = Env()
    e.log = []
    monkeypatch.setattr(StubTokenizer, "log", e.log)
    monkeypatch.setattr(dictfile, "load_dict", lambda path: (e.log.append(("load", path)), StubDictFile())[1])
    monkeypatch.setattr(tokenizer, "Tokenizer", StubTokenizer)
    monkeypatch.setattr(vocab.Vocab, "from_words", staticmethod(lambda words, listed, unk, bos, eos: (e.log.append(("vocab", list(listed), unk, bos, eos)), StubVocab(e.log))[1]))
    e.vocab_file = str(tmp_path / "vocab.txt")
    with open(e.vocab_file, "wb") as f:
        f.write(b"<unk>\n<s>\nb\n")

    def run(argv, data=b""):
        args = cli.parse_args(argv)
        out = io.BytesIO()
        e.log.clear()
        status = getattr(cli, args.command)(args, io.BytesIO(data), out)
        return status, out.getvalue()

    e.run = run
    return e


GOOD = [b"a b", b"", b"cc d  ", b"e", b"ff g h", b"i", b"jj", b"k l", b"m", b"n o p", b"qq", b"r s", b"t", b"u v"]   # (split_lines trims the trailing blanks)
BAD_AT = 4                                                                        # 0-based: with 16-byte blocks the second block holds it
COMMANDS = {
    "tokenize": ([], lambda ln: ln + b"\tX\nEOS\n"),
    "wakati": ([], lambda ln: ln + b"\n"),
    "encode": (None, lambda ln: " ".join(str(len(w)) for w in ln.split()).encode() + b"\n"),
}


def _argv(cli_env, command, *more):
    return [command, "-c", "some.dict", "--block-bytes", "16"] + (["--vocab", cli_env.vocab_file] if command == "encode" else []) + list(more)


def _expected(command, lines):
    trimmed = [ln.rstrip() for ln in lines]
    if command == "count":
        seen = Counter(w for ln in trimmed if _valid(ln) for w in ln.split())
        return b"".join(b"%d\t%s\n" % (n, w) for w, n in sorted(seen.items(), key=lambda kv: (-kv[1], kv[0])))
    return b"".join(COMMANDS[command][1](ln) for ln in trimmed if _valid(ln))


@pytest.mark.parametrize("command", ["tokenize", "wakati", "count", "encode"])
def test_cli_input_forms_print_the_same(cli_env, command):
    data = b"\n".join(GOOD) + b"\n"
    status, host = cli_env.run(_argv(cli_env, command), data)
    assert status == 0 and cli_env.log.count("packed") >= 3 and "text" not in cli_env.log     # three blocks or more
    assert cli_env.log[:3] == [("load", "some.dict"), "open", "features"]
    assert host == _expected(command, GOOD)
    status, device = cli_env.run(_argv(cli_env, command, "--split", "device"), data)
    assert status == 0 and cli_env.log.count("text") == host_blocks(data) and "packed" not in cli_env.log and device == host
    # an INPUT argument is one sentence, untrimmed, and stdin is not read
    status, one = cli_env.run(_argv(cli_env, command, "k l"), b"never read\n")
    assert status == 0 and cli_env.log.count("packed") == 1 and one == cli_env.run(_argv(cli_env, command), b"k l\n")[1] == _expected(command, [b"k l"])
    # the last line may lack its newline; no input at all prints nothing
    assert cli_env.run(_argv(cli_env, command), data[:-1])[1] == host
    assert cli_env.run(_argv(cli_env, command), b"") == (0, b"")


def host_blocks(data, block_bytes=16):
    from kanpyo_amd.cli import _blocks

    return len(list(_blocks(io.BytesIO(data), block_bytes)))


@pytest.mark.parametrize("split", ["host", "device"])
@pytest.mark.parametrize("command,text", [("tokenize", "thread 'main' panicked: failed to read from stdin: stream did not contain valid UTF-8\n"),
                                          ("wakati", "kanpyo_amd: failed to read from stdin: stream did not contain valid UTF-8\n")])
def test_cli_tokenize_and_wakati_stop_at_a_bad_line(cli_env, capsys, command, text, split):
    lines = list(GOOD)
    lines[BAD_AT] = b"\xff\xfe x"
    status, out = cli_env.run(_argv(cli_env, command, "--split", split), b"\n".join(lines) + b"\n")
    assert status == 101 and out == _expected(command, lines[:BAD_AT]) and out
    assert cli_env.log.count("packed" if split == "host" else "text") == 2 < host_blocks(b"\n".join(lines) + b"\n")   # (in the second block; no third is read)
    assert capsys.readouterr().err == text


@pytest.mark.parametrize("split", ["host", "device"])
@pytest.mark.parametrize("command", ["count", "encode"])
def test_cli_count_and_encode_report_bad_lines(cli_env, capsys, command, split):
    lines = list(GOOD)
    lines[BAD_AT] = b"\xff\xfe x"
    lines[11] = b"\xe3\x81"
    data = b"\n".join(lines) + b"\n"
    status, out = cli_env.run(_argv(cli_env, command, "--split", split), data)
    assert (status, out) == (101, b"")
    assert capsys.readouterr().err == f"kanpyo_amd: line {BAD_AT + 1}: not valid UTF-8\n"
    status, out = cli_env.run(_argv(cli_env, command, "--split", split, "--skip-invalid"), data)
    assert status == 0
    assert capsys.readouterr().err == f"kanpyo_amd: line {BAD_AT + 1}: not valid UTF-8 (skipped)\nkanpyo_amd: line 12: not valid UTF-8 (skipped)\n"
    if command == "count":
        assert out == _expected("count", lines)
    else:   # (a skipped line prints an empty line: the stub adds no bos / eos)
        assert out == b"".join(COMMANDS["encode"][1](ln.rstrip()) if _valid(ln) else b"\n" for ln in lines)


def test_cli_options_reach_the_handles(cli_env):
    cli_env.run(_argv(cli_env, "wakati", "--base-form", "--drop", "助詞,記号", "--separator", "/"), b"a\n")
    assert ("words", 6, ["助詞", "記号"], [], b"/") in cli_env.log
    cli_env.run(_argv(cli_env, "count", "--field", "2", "--keep", "名詞", "--top", "1"), b"a\n")
    assert ("words", 2, [], ["名詞"], " ") in cli_env.log
    assert cli_env.run(_argv(cli_env, "count", "--top", "1"), b"a b\nb\n")[1] == b"2\tb\n"
    cli_env.run(_argv(cli_env, "encode", "--reading", "--bos", "<s>"), b"a\n")
    assert ("words", 7, [], [], " ") in cli_env.log and ("vocab", [b"<unk>", b"<s>", b"b"], b"<unk>", b"<s>", None) in cli_env.log


def test_cli_encode_checks_its_vocabulary_before_any_dictionary(cli_env, capsys):
    assert cli_env.run(_argv(cli_env, "encode", "--bos", "<bos>"), b"a\n") == (2, b"")
    assert cli_env.log == [] and capsys.readouterr().err == f"kanpyo_amd: --bos '<bos>' is not a line of {cli_env.vocab_file}\n"
    argv = ["encode", "-c", "some.dict", "--vocab", cli_env.vocab_file + ".missing"]
    assert cli_env.run(argv, b"a\n") == (2, b"") and cli_env.log == []
    assert capsys.readouterr().err.startswith("kanpyo_amd: --vocab: ")


def test_cli_default_dictionary_path(cli_env, monkeypatch):
    from kanpyo_amd import cli

    monkeypatch.setenv("XDG_CONFIG_HOME", "/somewhere/absolute")
    for command in ("tokenize", "wakati", "count"):
        cli_env.run([command], b"")
        assert cli_env.log[0] == ("load", "/somewhere/absolute/kanpyo/ipa.dict") == ("load", cli.default_dict_path())
