"""What runs a batch of sentences on the device against the oracle, for every test of the tokenize kernels (pool, windowed, general): the `libs`
fixture, the launch-chain environment, ONE device-path harness (device_batch: torch-owned HBM buffers through a DeviceContext), ONE host-path
harness (host_batch: Tokenizer.tokenize_packed), and the thin wrappers over them.  Records, offsets and status are the oracle's bit for bit -- integer
work, no tolerance -- and a mismatch names the first differing token, its sentence and both records.

Needs a device when called, never at import (tests/kernel_cases.py, tests/window_cases.py and tests/pool_cases.py hold what is known before a GPU is
touched).  The asserts here are not rewritten by pytest: each carries its values in its message."""
import numpy as np
import pytest

from kernel_cases import CHAIN_KNOBS

# the routing counters the pool tests compare with tests/pool_model.py's prediction, and those the window tests compare between two runs
COUNTERS = ("deferred", "redone", "window_handed", "tail_reruns", "window_reruns", "arena_regrows")
ROUTING_KEYS = ("deferred", "redone", "window_handed", "tail_reruns", "arena_regrows", "window_reruns", "long_launches")
STATUS_MARKER = 0xEE   # what the status buffer holds before a batch: the kernels must have written every 0 themselves


@pytest.fixture(scope="module")
def libs():
    """(kanpyo_amd._lib, oracle) with the oracle built; a test module imports it (`from kernel_run import libs  # noqa: F401`) and keeps its own instance"""
    from kanpyo_amd import _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    from oracle import oracle

    oracle.build()
    return _lib, oracle


def set_env(monkeypatch, env, knobs=CHAIN_KNOBS):
    """clear the launch-chain knobs, then set this plan's (a Tokenizer / DeviceContext made afterwards reads them)"""
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _name(sentences, s):
    if sentences is None:
        return "of the packed batch"
    return repr(sentences[s]) if len(sentences[s]) <= 80 else f"{sentences[s][:24]!r}... of {len(sentences[s])} characters"


def assert_records(status, toff, tokens, exp, sentences, what=""):
    """status all zero, token offsets and records the oracle's (`exp`: OracleTokenizer.tokenize_batch's result, or anything with its .tokens and
    .offsets).  tokens: TOKEN_DTYPE records or rows of six int32; sentences: the batch, to name a sentence by its text, or None."""
    pre = f"{what}: " if what else ""
    n = len(exp.offsets) - 1 if sentences is None else len(sentences)
    status, toff = np.asarray(status), np.asarray(toff).astype(np.uint64)
    assert status.shape == (n,), f"{pre}{status.shape} status bytes for {n} sentences"
    assert not status.any(), f"{pre}status not zero: sentences {status.nonzero()[0][:8].tolist()} have {status[status.nonzero()[0][:8]].tolist()}"
    assert toff.shape == exp.offsets.shape, f"{pre}{toff.shape} token offsets, the oracle has {exp.offsets.shape}"
    if not np.array_equal(toff, exp.offsets):
        s = max(int(np.nonzero(toff != exp.offsets)[0][0]) - 1, 0)   # offset s + 1 is where sentence s ends
        raise AssertionError(f"{pre}per-sentence token counts differ, first at sentence {s} ({_name(sentences, s)}): gpu offsets "
                             f"{toff[s:s + 2].tolist()} oracle {exp.offsets[s:s + 2].tolist()}")
    got = np.ascontiguousarray(tokens).view(np.int32).reshape(-1, 6)
    want = exp.tokens.view(np.int32).reshape(-1, 6)
    assert got.shape == want.shape, f"{pre}{len(got)} records, the oracle has {len(want)}"
    if not np.array_equal(got, want):
        bad = int(np.nonzero((got != want).any(axis=1))[0][0])
        s = int(np.searchsorted(exp.offsets, bad, side="right") - 1)
        raise AssertionError(f"{pre}token {bad} (sentence {s}: {_name(sentences, s)}) differs: gpu {got[bad]} oracle {want[bad]}")


def device_batch(ctx, orc, sentences, exp=None, nthreads=2, what=""):
    """One batch through the device API on `ctx`: pack, upload, ctx.tokenize, ctx.sync; records, offsets and status must be the oracle's (computed on
    `nthreads` threads unless `exp` is given).  The status buffer starts as STATUS_MARKER; an empty batch or empty text gets a byte to point at.
    -> (token count, oracle result)"""
    import torch

    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sentences)
    if exp is None:
        exp = orc.tokenize_batch(utf8, offs, nthreads)
    dev = torch.device("cuda", 0)
    n, cap = len(sentences), int(offs[-1]) + len(sentences)
    d_utf8 = torch.from_numpy(utf8.copy()).to(dev) if utf8.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), STATUS_MARKER, dtype=torch.uint8, device=dev)
    ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
    nt = ctx.sync()
    assert_records(d_st[:n].cpu().numpy(), d_toff.cpu().numpy(), d_tok[:nt].cpu().numpy(), exp, sentences, what)
    return nt, exp


def host_batch(tok, orc, sentences, nthreads=2, what=""):
    """The same through the host-buffer entry point (Tokenizer.tokenize_packed).  -> oracle result"""
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sentences)
    exp = orc.tokenize_batch(utf8, offs, nthreads)
    got_t, got_off, status = tok.tokenize_packed(utf8, offs)
    assert_records(status, got_off, got_t, exp, sentences, what)
    return exp


def run_fresh(tok, orc, sentences, mode=None, nthreads=2, exp=None, also=()):
    """A fresh context on `tok` in profiling mode `mode` (PROFILE_OFF unless given), one batch (device_batch).  -> its profile(); with `also`
    (names of DeviceContext methods: "work", "plan") -> (profile, *those), each read before the profile"""
    from kanpyo_amd.device import PROFILE_OFF, DeviceContext

    ctx = DeviceContext(tok)
    try:
        ctx.set_profiling(PROFILE_OFF if mode is None else mode)
        device_batch(ctx, orc, sentences, exp, nthreads)
        extra = [getattr(ctx, name)() for name in also]
        prof = ctx.profile()
    finally:
        ctx.close()
    return (prof, *extra) if also else prof


def run_case(case, oracle, monkeypatch):
    """every batch of a tests/pool_cases.py case on a fresh handle: the oracle's records, the model's counters"""
    from kanpyo_amd import Dict, Tokenizer

    set_env(monkeypatch, case.env)
    d = Dict.from_parts(**case.parts)
    orc = oracle.OracleTokenizer.from_dict(d)
    for b in case.batches:
        tok = Tokenizer(d)
        try:
            prof = run_fresh(tok, orc, b.sentences)
        finally:
            tok.close()
        got, want = {k: prof[k] for k in COUNTERS}, b.expect()
        print(f"{case.name} [{b.note}] {len(b.sentences)} sentences: {got}")
        assert got == want, (case.name, b.note, got, want)


def run_batch(ctx, orc, sentences, exp=None):
    """One batch on `ctx` (a context that lives on between batches).  -> (routing counters of this batch, oracle result)"""
    _, exp = device_batch(ctx, orc, sentences, exp, nthreads=8)
    p = ctx.profile(reset=True)
    return {k: p[k] for k in ROUTING_KEYS}, exp


def run_scenario(sc, team, monkeypatch):
    """A tests/window_cases.py scenario's sentences one by one between ordinary ones (their own workgroups in a batch this small;
    test_the_next_sentence_of_a_workgroup puts a workgroup's next sentence behind a handed one), each batch twice on one context."""
    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import DeviceContext
    from window_cases import ORDINARY

    orc = sc.oracle()
    set_env(monkeypatch, dict({"KGPU_POOL": "0", "KGPU_WINDOW_TEAM": "2" if team else "0"}, **sc.env))
    tok = Tokenizer(sc.dict)
    ctx = DeviceContext(tok)
    assert ctx.plan()["window_lds_bytes"] == sc.lds, (sc.name, ctx.plan()["window_lds_bytes"], sc.lds)
    for special in sc.sentences:
        batch = ORDINARY[:3] + [special] + ORDINARY[3:] + [special] + ORDINARY[:2]
        first, exp = run_batch(ctx, orc, batch)
        again, _ = run_batch(ctx, orc, batch, exp)
        assert first == again, (sc.name, first, again)
        print(f"{sc.name} ({'team' if team else 'ordinary'} form), {len(special)} characters x 2: {first}")
        zero, want = [0] * 10, [0] * 4   # (every special sentence is in the batch twice)
        if team and sc.team_why:         # the team hands them to the ordinary form behind it (list 0) ...
            zero[sc.team_why] += 2
            want[0] = 2
        if sc.why:                       # ... which hands them on as well (list 1 then), or is the only form (list 0)
            zero[sc.why] += 2
            want[1 if team else 0] = 2
        assert first["window_handed"] == zero and first["deferred"] == want, (sc.name, team, first, zero, want)
        assert first["window_reruns"] == 0 and first["arena_regrows"] == 0 and first["tail_reruns"] == (1 if want[1 if team else 0] else 0), (sc.name, first)   # (the chain ends on list 1 behind the team, on list 0 without)
    ctx.close()
    tok.close()
