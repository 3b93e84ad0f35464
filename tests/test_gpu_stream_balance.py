"""Batches spread over the dictionary's shared streams by load (kanpyo_amd/csrc/kgpu_ctx.cpp: ctx_begin_batch over kgpu_chain.cpp: pick_stream): a context
created without a stream runs each batch on the least-loaded shared stream.  Which stream a batch was given is read from the per-dictionary witness
(kgpu_debug_stream_batches, tests only: not in the header), not assumed.

(a) eight contexts, 48 equal batches from one thread in the order bench_engine.GpuEngine keeps (sync the context's previous batch, then enqueue): the host's
    view of what is in flight is deterministic there -- a batch leaves the count only at its own context's sync -- so the streams' shares differ by at most 1;
(b) one context, 12 batches: it visits every shared stream;
(c) host-buffer calls from four threads on pooled contexts: the single-thread results, and one batch counted per call;
(d) a context on a caller-owned stream: never counted, never moved.
Every batch is compared bit-exactly with the oracle.  Batches of 64 short sentences over a small synthetic dictionary."""
import ctypes as C
import threading
import types

import numpy as np
import pytest

from kernel_run import assert_records, libs  # noqa: F401  (libs: the fixture)

pytestmark = pytest.mark.gpu

N = 64


@pytest.fixture(scope="module")
def env(libs):
    from kanpyo_amd import Tokenizer, synth
    from kanpyo_amd.tokenizer import pack_sentences

    _, oracle = libs
    sd = synth.build_dict(5000, seed=11)
    tok, orc = Tokenizer(sd.dict), oracle.OracleTokenizer.from_dict(sd.dict)
    sents = synth.make_corpus(sd, N * 5, 23, "cfg2")
    batches = []   # (utf8, offsets, expected tokens, expected offsets): computed once, left unchanged
    for k in range(5):
        u, o = pack_sentences(sents[k * N:(k + 1) * N])
        e = orc.tokenize_batch(u, o, 1)
        for a in (u, o, e.tokens, e.offsets):
            a.setflags(write=False)
        batches.append((u, o, e.tokens, e.offsets))
    yield tok, batches
    tok.close()


def _witness(tok, reset=False):
    """batches given to each shared stream of the tokenizer's dictionary since the last reset"""
    from kanpyo_amd import _lib

    f = _lib.lib().kgpu_debug_stream_batches
    f.argtypes, f.restype = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int], C.c_int
    out = (C.c_uint64 * 64)()
    n = int(f(tok.handle, out, 64, 1 if reset else 0))
    assert 0 <= n <= 64, n
    return [int(out[k]) for k in range(n)]


class _Slot:
    """A device context with the HBM buffers of one batch shape."""

    def __init__(self, tok, batch, stream_ptr=None):
        import torch

        from kanpyo_amd.device import DeviceContext

        dev = torch.device("cuda", 0)
        u, o, _, _ = batch
        self.n, self.total = len(o) - 1, int(o[-1])
        self.cap = self.total + self.n + 1
        self.d_utf8 = torch.from_numpy(np.concatenate([u, np.zeros(1, np.uint8)])).to(dev)
        self.d_off = torch.from_numpy(o.astype(np.int64)).to(dev)
        self.d_rec = torch.zeros((self.cap, 6), dtype=torch.int32, device=dev)
        self.d_toff = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.d_st = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)   # (the uploads ran on torch's stream: the contexts' streams do not wait for it)
        self.ctx = DeviceContext(tok, stream_ptr)
        self.torch, self.busy = torch, False

    def enqueue(self):
        self.ctx.tokenize(self.d_utf8.data_ptr(), self.d_off.data_ptr(), self.n, self.total, self.d_rec.data_ptr(), self.cap,
                          self.d_toff.data_ptr(), self.d_st.data_ptr())
        self.busy = True

    def collect(self, batch, what):
        _, _, etok, eoff = batch
        nt = self.ctx.sync()
        self.busy = False
        assert nt == len(etok), (what, nt, len(etok))
        assert_records(self.d_st.cpu().numpy(), self.d_toff.cpu().numpy(), self.d_rec[:nt].cpu().numpy(), types.SimpleNamespace(tokens=etok, offsets=eoff), None, what)
        self.d_rec.zero_()   # the next batch on this slot has to write them again (waited for here: the contexts' streams do not wait for torch's)
        self.d_toff.zero_()
        self.torch.cuda.synchronize(self.d_rec.device)

    def close(self):
        self.ctx.close()


def test_eight_contexts_share_the_streams_evenly(env):
    tok, batches = env
    slots = [_Slot(tok, batches[0]) for _ in range(8)]
    try:
        streams = slots[0].ctx.plan()["streams"]
        _witness(tok, reset=True)
        for b in range(48):
            s = slots[b % 8]
            if s.busy:
                s.collect(batches[0], f"batch {b - 8}")
            s.enqueue()
        for i, s in enumerate(slots):
            s.collect(batches[0], f"batch {40 + i}")
        got = _witness(tok)
        assert len(got) == streams and sum(got) == 48, (got, streams)
        assert max(got) - min(got) <= 1, got
    finally:
        for s in slots:
            s.close()


def test_one_context_visits_every_stream(env):
    tok, batches = env
    s = _Slot(tok, batches[1])
    try:
        _witness(tok, reset=True)
        for b in range(12):
            s.enqueue()
            s.collect(batches[1], f"batch {b}")
        got = _witness(tok)
        assert len(got) == s.ctx.plan()["streams"] and sum(got) == 12 and min(got) >= 1, got
    finally:
        s.close()


def test_host_calls_from_four_threads(env, monkeypatch):
    tok, batches = env
    monkeypatch.setenv("KGPU_NO_SMALL_CALLS", "1")   # 64 sentences would be one small launch: the chunked path on pooled contexts, one batch a call
    single = []
    for u, o, etok, eoff in batches[1:]:
        t, toff, st = tok.tokenize_packed(u, o)
        assert not st.any() and np.array_equal(toff, eoff) and np.array_equal(t, etok)
        single.append((t.copy(), toff.copy()))
    _witness(tok, reset=True)
    calls, errors = 6, []
    start = threading.Barrier(4)

    def body(t):
        try:
            u, o, _, _ = batches[1 + t]
            start.wait()
            for k in range(calls):
                got_t, got_o, st = tok.tokenize_packed(u, o)
                if st.any() or not np.array_equal(got_o, single[t][1]) or not np.array_equal(got_t, single[t][0]):
                    errors.append((t, k))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    ths = [threading.Thread(target=body, args=(t,)) for t in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors
    got = _witness(tok)
    assert sum(got) == 4 * calls, got


def test_caller_stream_is_left_alone(env):
    import torch

    tok, batches = env
    _Slot(tok, batches[0]).close()   # (the shared streams exist: the witness has its entries)
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    s = _Slot(tok, batches[2], st.cuda_stream)
    try:
        before = _witness(tok, reset=True)
        assert len(before) == s.ctx.plan()["streams"], before
        for b in range(4):
            s.enqueue()
            s.collect(batches[2], f"batch {b}")
        got = _witness(tok)
        assert len(got) == len(before) and not any(got), got
    finally:
        s.close()
