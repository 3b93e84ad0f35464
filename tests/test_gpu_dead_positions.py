"""Dead positions in the pool kernel (kanpyo_amd/csrc/kgpu_pool.hip): a start position nothing ends at (P = 0) has no stage-B tile -- the emit phase
writes its nodes' result (dp = INF, no best predecessor) -- bit-exact against the oracle on lattices whose dead positions are known by construction.

The dictionary has "あいう" x 2, "い" x k, "う" x 3 and hiragana unknown words that group: in "あいう" nothing ends at position 1, so its k + 1 nodes
("い" x k and the unknown "いう") are dead: (T, P) = (k + 1, 0); position 2 has P = k, every one of them a dead node, and four live targets.  With
k in 1, 7, 8, 9, 16, 17 the dead position would have been 1, 2 and 3 target groups (T on both sides of 8 and 16) and the all-dead bucket behind it
crosses the chunk size.  The shapes are checked here with the naive restatement (oracle/pyref.py) before anything runs on the GPU.

A second dictionary has the costs of test_gpu_parity.py::test_unreachable_eos_and_dead_ends (matrix entries of -30000, a word cost of -20000) and
no unknown word for katakana: behind "テ" every node is unreachable, INF + cost + matrix < INF lets a dead predecessor win, and the best path ENDS in
a dead node (its tokens start in the middle of the sentence) -- or EOS itself is dead and the result is empty.

Plans: the shipped chain and a 160 KB pool through a device context (that the pool kernel served the batch is asserted from the routing counters, as
in test_gpu_tile_groups.py), and kgpu_tokenize_batch with at most 128 sentences: the single-launch small call, the same kernel with one wavefront a
workgroup."""
import numpy as np
import pytest

import pool_model as M
from kernel_cases import BASES, BEHIND_TE, DEAD_ENDS, MODEL_PLANS, PLANS, dead_model, dead_need, dead_parts, dead_sentences
from kernel_run import host_batch, libs, run_fresh, set_env  # noqa: F401  (libs: the fixture)
from pool_model import shape as _shape

pytestmark = pytest.mark.gpu

KS = [1, 7, 8, 9, 16, 17]
PLAN_NAMES = ["shipped", "pool160x4", "small"]
SHIPPED_CHARS = 36   # what the shipped plan's pool kernel is asserted to serve itself (see kernel_cases.dead_need)


def _dict(k, negative=False):
    from kanpyo_amd import Dict

    return Dict.from_parts(**dead_parts(k, negative))


def _pyref(d):
    from oracle import pyref

    return pyref, pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)


def _check_small(tok, orc, sentences):
    """kgpu_tokenize_batch in calls of at most 100 sentences and well below 16 KB: the single-launch small call"""
    for i0 in range(0, len(sentences), 100):
        part = sentences[i0:i0 + 100]
        assert len(part) <= 128 and sum(len(s.encode()) for s in part) < 16 * 1024
        host_batch(tok, orc, part)


def _set_plan(monkeypatch, plan):
    set_env(monkeypatch, PLANS[plan][0] if plan in PLANS else {})


def _check(tok, orc, plan, alone, batch, inside, monkeypatch, d, model):
    """every sentence of `alone` in a batch of its own, then `batch` in one; on the device-context plans the sentences for which `inside` holds must have
    been served by the pool kernel, the rest run with the windowed kernel behind it and must not reach the general kernel.  The redo and hand-on counts
    are the reservation model's (tests/pool_model.py), exactly: `tok` is a fresh handle, every batch on it steps the estimate by the restated rule of
    chain_feedback (M.steer: a batch of one sentence without a redo takes 1/128 off), and every batch runs on a context of its own, so the shipped plan's
    pool keeps its 40 KB shape (kernel_cases.MODEL_PLANS)."""
    from kanpyo_amd import Tokenizer

    if plan == "small":
        for s in alone:
            _check_small(tok, orc, [s])
        _check_small(tok, orc, batch)
        return
    est = M.EST_Q8_FRESH

    def predicted(sentences, est_q8):
        return M.counters([model.verdict(s, MODEL_PLANS[plan], est_q8)["verdict"] for s in sentences])

    for s in alone:
        prof = run_fresh(tok, orc, [s])
        want = predicted([s], est)
        assert sum(prof["deferred"]) == 0 and want[0] == 0, (s, prof)   # the pool kernel served it
        assert prof["redone"][0] == want[1], (s, want, prof)
        est = M.steer(est, want[1], 1)
    ins = [s for s in batch if inside(s)]
    beyond = [s for s in batch if not inside(s)]
    prof = run_fresh(tok, orc, ins)
    want = predicted(ins, est)
    print(f"{plan}: {len(ins)} sentences meant for the pool kernel: deferred {prof['deferred']} redone {prof['redone']} (est_q8 {est}); {len(beyond)} beyond")
    assert sum(prof["deferred"]) == 0 and want[0] == 0 and prof["redone"][0] == want[1], (want, prof)
    if beyond:
        monkeypatch.setenv("KGPU_WINDOW", "24")
        tok2 = Tokenizer(d)
        try:
            prof = run_fresh(tok2, orc, beyond)
        finally:
            tok2.close()
        want = predicted(beyond, M.EST_Q8_FRESH)   # (a fresh handle)
        assert prof["deferred"][0] == want[0] <= len(beyond) and sum(prof["deferred"][1:]) == 0 and prof["redone"][0] == want[1], (want, prof)


@pytest.mark.parametrize("plan", PLAN_NAMES)
@pytest.mark.parametrize("k", KS)
def test_dead_positions(libs, k, plan, monkeypatch):
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    d = _dict(k)
    pyref, pd = _pyref(d)
    # the shapes, by the naive lattice: position 1 of "あいう" is dead with k + 1 targets, position 2 has the k dead nodes as its only predecessors
    for s, at in (("あいう", 0), ("あいうあいう", 0), ("あいうあいう", 3), ("いあいう", 1), ("あいういう", 0)):
        tp, nodes, dp, pre = _shape(pyref, pd, s)
        assert tp[at + 1] == (k + 1, 0) and tp[at + 2] == (4, k), (s, at, tp)
        dead = [i for i, n in enumerate(nodes) if n[3] == at + 1]
        assert all(dp[i] == 1 << 30 and pre[i] is None for i in dead)
    assert _shape(pyref, pd, "あいういう")[0][3] == (k + 1, 5)   # ... and a live position with the same targets beside it
    limit = 32 * 624 if plan == "shipped" else 64 * 2544
    assert all(dead_need(pyref, pd, b * (SHIPPED_CHARS // len(b))) * 6 <= 32 * 624 * 5 for b in BASES)
    assert all(dead_need(pyref, pd, b * 12 + "あ") * 6 <= 64 * 2544 * 5 for b in BASES)
    inside = (lambda s: len(s) <= SHIPPED_CHARS) if limit == 32 * 624 else (lambda s: True)
    _set_plan(monkeypatch, plan)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    try:
        _check(tok, orc, plan, BASES, dead_sentences(np.random.default_rng(k)), inside, monkeypatch, d, dead_model(k))
    finally:
        tok.close()


@pytest.mark.parametrize("plan", PLAN_NAMES)
@pytest.mark.parametrize("k", KS)
def test_dead_positions_negative_costs(libs, k, plan, monkeypatch):
    """INF + cost + matrix < INF: a dead node wins as a predecessor and the best path ends in it; EOS itself dead: no token."""
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    d = _dict(k, negative=True)
    pyref, pd = _pyref(d)
    tp, nodes, dp, pre = _shape(pyref, pd, "テいう")
    assert tp[0] == (0, 1) and tp[1] == (k + 1, 0) and tp[2] == (4, k) and tp[3][0] == 1, tp
    toks = pyref.tokenize(pd, "テいう")
    assert len(toks) == 2 and toks[0][3] == 2 and toks[1][1] == 0, toks   # "う", EOS: the path's first node hangs on a dead "い" and starts at 2
    last = len(nodes) - 1
    assert dp[pre[last]] < (1 << 30) - 40000 and pre[pre[pre[last]]] is None and nodes[pre[pre[last]]][3] == 1
    assert pyref.tokenize(pd, "テ") == [] and pyref.tokenize(pd, "テあ") == []   # nothing ends at C / only unreachable nodes do
    _set_plan(monkeypatch, plan)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    rng = np.random.default_rng(100 + k)
    batch = dead_sentences(rng) + DEAD_ENDS + BEHIND_TE + [a + b for a in BEHIND_TE for b in DEAD_ENDS[:4]]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    inside = (lambda s: len(s) <= SHIPPED_CHARS) if plan == "shipped" else (lambda s: True)
    try:
        _check(tok, orc, plan, BASES + DEAD_ENDS + BEHIND_TE, batch, inside, monkeypatch, d, dead_model(k, True))
    finally:
        tok.close()


@pytest.mark.parametrize("plan", ["shipped", "pool160x4"])
@pytest.mark.parametrize("k", [1, 17])
def test_many_dead_positions_long_sentence(libs, k, plan, monkeypatch):
    """40 x "あいう": 40 dead positions in one sentence, in a batch with short ones, the windowed kernel off -- the pool kernel serves it or routes it to
    the general kernel, and the records are the oracle's either way."""
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    _set_plan(monkeypatch, plan)
    monkeypatch.setenv("KGPU_WINDOW", "0")
    for negative in (False, True):
        d = _dict(k, negative)
        tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
        try:
            prof = run_fresh(tok, orc, ["あいう" * 40, "あいう", ("テ" if negative else "") + "あいういう" * 24, "いあいう" * 3, ""])
            print(f"k={k} {plan} negative={negative}: deferred {prof['deferred']} redone {prof['redone']} long_launches {prof['long_launches']}")
        finally:
            tok.close()
