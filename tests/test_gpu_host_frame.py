"""The frame the eight chunked host calls share -- kgpu_tokenize_batch_lines / _words, kgpu_encode_batch, kgpu_count_batch over a packed batch and
kgpu_tokenize_text_lines / _words, kgpu_encode_text, kgpu_count_text over a raw block -- as one cross-product: every form in chunks of one and two
lines on a ring that wraps, against the same call in one chunk; each text form against its packed form; the empty call; the overflow protocols
with a buffer that holds the first chunk and not the second; and after every call, the failing ones included, the pooled contexts idle again
(a plain tokenize_packed gives the oracle's tokens).  What each renderer writes is the per-feature files' business (test_gpu_lines, _words,
_encode, _count); here a form is only ever compared with itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = ("lines", "words", "ids")
CHUNKED = [{"KGPU_HOST_CHUNK_SENTS": s, "KGPU_HOST_DEPTH": "3"} for s in ("1", "2")]   # (the batch ring has three jobs, the text ring four: seven lines wrap both)
SENTINEL = 0xEE


class Env:
    def __init__(self):
        from kanpyo_amd import Tokenizer, synth
        from kanpyo_amd.tokenizer import pack_sentences, split_lines
        from oracle import oracle

        oracle.build()
        sd = synth.build_dict(20000, seed=11)
        known, unk = synth.feature_tables(sd)
        self.tok = Tokenizer(sd.dict)
        self.tok.set_features(known, unk)
        five = [s.encode("utf-8") for s in synth.make_corpus(sd, 5, 3, "cfg2")]
        self.lines = five[:2] + [b""] + five[2:3] + [b"\xe3\x81"] + five[3:]   # seven: one empty, one not UTF-8
        self.block = b"\n".join(self.lines)
        self.packed = split_lines(self.block)
        assert pack_sentences(self.lines)[0].tobytes() == self.packed[0].tobytes() and len(self.packed[1]) == 8
        self.n = 7
        # what a plain tokenize gives while the contexts are in order: the oracle's records of the valid lines, nothing for the other
        orc = oracle.OracleTokenizer.from_dict(sd.dict)
        valid = [s for s in self.lines if s != b"\xe3\x81"]
        exp = orc.tokenize_batch(*pack_sentences(valid), 1)
        self.want_tokens = exp.tokens
        self.want_status = [0, 0, 0, 0, 1, 0, 0]
        self.words = self.tok.words()
        listed = sorted({w for line in self.words.render(five[:3]) for w in line.encode("utf-8").split(b" ") if w})
        self.vocab = self.words.vocabulary([b"<unk>", b"</s>"] + listed, 0, None, 1)   # (eos: every valid line has an id, the words of two lines are unlisted)

    def idle(self):
        """Item 5: the contexts went back to the pool idle."""
        t, toff, status = self.tok.tokenize_packed(*self.packed)
        assert status.tolist() == self.want_status
        assert np.array_equal(t, self.want_tokens) and int(toff[-1]) == len(self.want_tokens)

    def packed_call(self, form, utf8, offs):
        call = {"lines": self.tok.tokenize_lines_packed, "words": self.words.render_packed, "ids": self.vocab.encode_packed}[form]
        return call(utf8, offs)

    def text_call(self, form, block):
        call = {"lines": self.tok.tokenize_text_lines, "words": self.words.render_text, "ids": self.vocab.encode_text}[form]
        return call(block)

    def entry(self, form, text):
        from kanpyo_amd import _lib

        L = _lib.lib()
        name = {("lines", False): "kgpu_tokenize_batch_lines", ("words", False): "kgpu_tokenize_batch_words", ("ids", False): "kgpu_encode_batch",
                ("lines", True): "kgpu_tokenize_text_lines", ("words", True): "kgpu_tokenize_text_words", ("ids", True): "kgpu_encode_text"}[(form, text)]
        handle = {"lines": self.tok, "words": self.words, "ids": self.vocab}[form].handle
        return getattr(L, name), handle, np.int32 if form == "ids" else np.uint8

    def counted(self, add, arg):
        k = self.words.counter(table_slots=1 << 10, key_bytes=1 << 16)
        status = getattr(k, add)(*arg)
        got = (status.tolist(), k.most_common(), k.info()["tokens_counted"])
        k.close()
        return got


@pytest.fixture(scope="module")
def env():
    return Env()


def same(a, b, what):
    for x, y, part in zip(a, b, ("units", "offsets", "status")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, part)


def setenv(monkeypatch, hooks):
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)


def clearenv(monkeypatch, hooks):
    for k in hooks:
        monkeypatch.delenv(k)


@pytest.mark.parametrize("hooks", CHUNKED, ids=["chunks-of-1", "chunks-of-2"])
@pytest.mark.parametrize("form", FORMS)
def test_chunked_equals_one_chunk_and_text_equals_packed(env, form, hooks, monkeypatch):
    whole_p = env.packed_call(form, *env.packed)
    env.idle()
    whole_t = env.text_call(form, env.block)
    env.idle()
    assert whole_p[2].tolist() == env.want_status and len(whole_p[0]) > 0
    same(whole_t, whole_p, "text form against packed form")
    setenv(monkeypatch, hooks)
    chunk_p = env.packed_call(form, *env.packed)
    chunk_t = env.text_call(form, env.block)
    clearenv(monkeypatch, hooks)
    env.idle()
    same(chunk_p, whole_p, "packed form in chunks")
    same(chunk_t, whole_p, "text form in chunks")


@pytest.mark.parametrize("hooks", CHUNKED, ids=["chunks-of-1", "chunks-of-2"])
def test_counts_chunked_equals_one_chunk_and_text_equals_packed(env, hooks, monkeypatch):
    whole_p = env.counted("add_packed", env.packed)
    env.idle()
    whole_t = env.counted("add_text", (env.block,))
    env.idle()
    assert whole_p[0] == env.want_status and whole_p[1] and whole_p[2] > 0
    assert whole_t == whole_p
    setenv(monkeypatch, hooks)
    chunk_p = env.counted("add_packed", env.packed)
    chunk_t = env.counted("add_text", (env.block,))
    clearenv(monkeypatch, hooks)
    env.idle()
    assert chunk_p == whole_p and chunk_t == whole_p


def test_empty_calls(env):
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import pack_sentences

    L = _lib.lib()
    none = pack_sentences([])
    for form in FORMS:
        for units, off, status in (env.packed_call(form, *none), env.text_call(form, b"")):
            assert len(units) == 0 and off.tolist() == [0] and len(status) == 0, form
        env.idle()
        # ... and the C calls themselves: KGPU_OK, the offsets table [0], nothing reported
        fn, h, dtype = env.entry(form, False)
        off, got = np.full(1, SENTINEL, dtype=np.uint64), C.c_uint64(SENTINEL)
        assert fn(h, None, none[1].ctypes.data, 0, None, 0, off.ctypes.data, None, C.byref(got)) == _lib.KGPU_OK
        assert off.tolist() == [0] and got.value == 0, form
        fn, h, dtype = env.entry(form, True)
        off, n, got = np.full(1, SENTINEL, dtype=np.uint64), C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
        assert fn(h, None, 0, None, 0, off.ctypes.data, 1, None, C.byref(n), C.byref(got)) == _lib.KGPU_OK
        assert off.tolist() == [0] and (n.value, got.value) == (0, 0), form
        env.idle()
    k = env.words.counter(table_slots=1 << 10, key_bytes=1 << 16)
    assert len(k.add_packed(*none)) == 0 and len(k.add_text(b"")) == 0
    n = C.c_uint64(SENTINEL)
    assert L.kgpu_count_batch(k.handle, None, none[1].ctypes.data, 0, None) == _lib.KGPU_OK
    assert L.kgpu_count_text(k.handle, None, 0, None, 0, C.byref(n)) == _lib.KGPU_OK and n.value == 0
    assert k.most_common() == [] and k.info()["tokens_counted"] == 0
    k.close()
    env.idle()


@pytest.mark.parametrize("form", FORMS)
def test_overflow_in_the_second_chunk(env, form, monkeypatch):
    from kanpyo_amd import _lib

    utf8, offs = env.packed
    n = env.n
    units, uoff, status = env.packed_call(form, utf8, offs)
    total, first = len(units), int(uoff[1])
    assert 0 < first < int(uoff[2]), "the first chunk writes something and so does the second"
    setenv(monkeypatch, CHUNKED[0])
    # packed: KGPU_ERR_CAPACITY, the exact size, all n status bytes
    fn, h, dtype = env.entry(form, False)
    buf, off, st, got = np.empty(first, dtype=dtype), np.empty(n + 1, dtype=np.uint64), np.full(n, SENTINEL, dtype=np.uint8), C.c_uint64(0)
    rc = fn(h, utf8.ctypes.data, offs.ctypes.data, n, buf.ctypes.data, first, off.ctypes.data, st.ctypes.data, C.byref(got))
    assert rc == _lib.KGPU_ERR_CAPACITY and got.value == total and st.tolist() == status.tolist()
    assert f"need {total}, capacity {first}" in L_error()
    env.idle()
    # ... and with the exact size the call goes through
    buf = np.empty(total, dtype=dtype)
    rc = fn(h, utf8.ctypes.data, offs.ctypes.data, n, buf.ctypes.data, total, off.ctypes.data, st.ctypes.data, C.byref(got))
    assert rc == _lib.KGPU_OK and got.value == total
    same((buf, off, st), (units, uoff, status), "exact capacity")
    # text: KGPU_ERR_CAPACITY, the exact sizes, n_lines set -- the text buffer short, then the offsets table one short
    fn, h, dtype = env.entry(form, True)
    src = np.frombuffer(env.block, dtype=np.uint8)
    for tcap, ocap in ((first, n + 1), (total, n)):
        buf, off, st = np.empty(total, dtype=dtype), np.empty(n + 1, dtype=np.uint64), np.full(n + 1, SENTINEL, dtype=np.uint8)
        lines, got = C.c_uint64(0), C.c_uint64(0)
        rc = fn(h, src.ctypes.data, src.size, buf.ctypes.data, tcap, off.ctypes.data, ocap, st.ctypes.data, C.byref(lines), C.byref(got))
        assert rc == _lib.KGPU_ERR_CAPACITY and (lines.value, got.value) == (n, total), (tcap, ocap)
        assert f"need {total} text bytes (capacity {tcap}) and {n + 1} offsets (capacity {ocap})" in L_error()
        env.idle()
    buf, off, st = np.empty(total, dtype=dtype), np.empty(n + 1, dtype=np.uint64), np.full(n, SENTINEL, dtype=np.uint8)
    rc = fn(h, src.ctypes.data, src.size, buf.ctypes.data, total, off.ctypes.data, n + 1, st.ctypes.data, C.byref(lines), C.byref(got))
    assert rc == _lib.KGPU_OK and (lines.value, got.value) == (n, total)
    same((buf, off, st), (units, uoff, status), "exact capacities")
    clearenv(monkeypatch, CHUNKED[0])
    env.idle()


def L_error():
    from kanpyo_amd import _lib

    return _lib.lib().kgpu_last_error().decode("utf-8", "replace")


def test_count_text_status_capacity_one_short_counts_nothing(env, monkeypatch):
    from kanpyo_amd import _lib

    n = env.n
    k = env.words.counter(table_slots=1 << 10, key_bytes=1 << 16)
    k.add_packed(*env.packed)
    before, common = k.info(), k.most_common()
    assert before["tokens_counted"] > 0
    src = np.frombuffer(env.block, dtype=np.uint8)
    setenv(monkeypatch, CHUNKED[0])
    st, lines = np.full(n, SENTINEL, dtype=np.uint8), C.c_uint64(0)
    rc = _lib.lib().kgpu_count_text(k.handle, src.ctypes.data, src.size, st.ctypes.data, n - 1, C.byref(lines))
    assert rc == _lib.KGPU_ERR_CAPACITY and lines.value == n and "nothing was counted" in L_error()
    assert k.info() == before and k.most_common() == common and (st == SENTINEL).all()
    env.idle()
    rc = _lib.lib().kgpu_count_text(k.handle, src.ctypes.data, src.size, st.ctypes.data, n, C.byref(lines))
    clearenv(monkeypatch, CHUNKED[0])
    assert rc == _lib.KGPU_OK and lines.value == n and st.tolist() == env.want_status
    assert k.info()["tokens_counted"] == 2 * before["tokens_counted"] and k.most_common() == [(w, 2 * c) for w, c in common]
    k.close()
    env.idle()
