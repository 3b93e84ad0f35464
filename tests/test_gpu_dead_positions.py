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
import functools

import numpy as np
import pytest

import pool_cases as PC
import pool_model as M
from conftest import fixture_dict_parts
from pool_model import shape as _shape
from test_gpu_tile_groups import MODEL_PLANS
from test_gpu_tile_groups import PLANS as TILE_PLANS
from test_gpu_tile_groups import _run

pytestmark = pytest.mark.gpu

KS = [1, 7, 8, 9, 16, 17]
BASES = ["あいう", "あいうあいう", "いあいう", "あいういう"]
ORDINARY = ["", "あ", "い", "う", "いう", "うい", "ういあ", "いいい", "あいあ", "ううう", "あい", "いあ"]
DEAD_ENDS = ["テ", "テあ", "テ辞書", "テ辞書形態素", "テスト辞書", "ト辞書あ", "辞書テ", "形態素テ形態素", "テテ辞書辞書"]   # test_unreachable_eos_and_dead_ends
BEHIND_TE = ["テいう", "テあいう", "テいうあいう", "テあいういう", "いうテいう", "テう", "テい"]
PLAN_NAMES = ["shipped", "pool160x4", "small"]
SHIPPED_CHARS = 36   # what the shipped plan's pool kernel is asserted to serve itself (see _need)


@pytest.fixture(scope="module")
def libs():
    from kanpyo_amd import _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    from oracle import oracle

    oracle.build()
    return _lib, oracle


def _parts(k, negative=False):
    kws = ["あいう"] * 2 + ["い"] * k + ["う"] * 3
    p = fixture_dict_parts()
    if not negative:
        rng = np.random.default_rng(2000 + k)
        # few distinct costs: ties between predecessors are common (first minimum in insertion order, lattice.rs:125,136)
        morphs = np.stack([rng.integers(0, 5, len(kws)), rng.integers(0, 5, len(kws)), rng.integers(-3, 4, len(kws)) * 100], axis=1)
        return dict(sorted_keywords=kws, morphs=morphs, conn_rows=5, conn_cols=5, conn_data=rng.integers(-2, 3, 25) * 50, char_class=p["char_class"],
                    char_category=p["char_category"], invoke_list=p["invoke_list"], group_list=p["group_list"], unk_map={0: (1, 1), 1: (1, 2), 2: (2, 1)},
                    unk_morphs=[[0, 0, 4000], [1, 1, 3500]])
    # the fixture's three words behind them (same first byte as the hiragana ones, then the kanji: the order the fixture itself has)
    three = [[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]]
    morphs = [three[i % 3] for i in range(2)] + [three[(i + 1) % 3] for i in range(k)] + [[1, 1, -20000], [2, 2, -20000], [0, 0, 1000]] + three
    p["sorted_keywords"] = kws + list(p["sorted_keywords"])
    p["morphs"] = morphs
    p["conn_data"] = [0, 100, 200, 100, -30000, 100, 200, 100, -30000]
    return p


def _dict(k, negative=False):
    from kanpyo_amd import Dict

    return Dict.from_parts(**_parts(k, negative))


@functools.lru_cache(maxsize=None)
def _model(k, negative=False):
    """the reservation model's view of this dictionary (tests/pool_model.py; tests/test_pool_model_cpu.py checks its shapes against the naive lattice)"""
    return PC.Dictionary(_parts(k, negative))


def _pyref(d):
    from oracle import pyref

    return pyref, pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)


def _need(pyref, pd, s):
    """Upper estimate of the pool kernel's LDS bytes for s, from the naive lattice: text, the per-character arrays, 12 bytes a node, 8 a bucket entry,
    8 a tile of a live position -- or, while the nodes are emitted, the match buffer (32 bytes a character) in the place of buckets and tiles."""
    tp, nodes, _, _ = _shape(pyref, pd, s)
    C, N = len(s), len(nodes)
    tiles = sum(((t + 7) // 8) * ((p + 7) // 8) for t, p in tp)
    return 3 * C + 4 + 26 * (C + 2) + 12 * (N + 1) + max(8 * (N + 1) + 8 * tiles, 32 * C + 32) + 64


def _sentences(rng):
    """about 200: the four shapes 1 to 12 times repeated, mixed with ordinary ones"""
    out = [b * r for b in BASES for r in range(1, 13)]
    out += [b * r + o for b in BASES for r in (1, 2, 5) for o in ("い", "う", "あ")]
    while len(out) < 200:
        out.append("".join(rng.choice(ORDINARY + BASES, size=int(rng.integers(1, 5)))))
    return [out[i] for i in rng.permutation(len(out))]


def _check_small(tok, orc, sentences):
    """kgpu_tokenize_batch in calls of at most 100 sentences and well below 16 KB: the single-launch small call"""
    from kanpyo_amd.tokenizer import pack_sentences

    for i0 in range(0, len(sentences), 100):
        part = sentences[i0:i0 + 100]
        utf8, offs = pack_sentences(part)
        assert len(part) <= 128 and int(offs[-1]) < 16 * 1024
        got_t, got_off, status = tok.tokenize_packed(utf8, offs)
        exp = orc.tokenize_batch(utf8, offs, 2)
        assert not status.any()
        assert np.array_equal(got_off, exp.offsets), "per-sentence token counts differ"
        if not np.array_equal(got_t, exp.tokens):
            bad = int(np.nonzero(got_t != exp.tokens)[0][0])
            s = int(np.searchsorted(exp.offsets, bad, side="right") - 1)
            raise AssertionError(f"token {bad} (sentence {s}: {part[s]!r}) differs: gpu {got_t[bad]} oracle {exp.tokens[bad]}")


def _set_plan(monkeypatch, plan):
    for name in ("KGPU_POOL", "KGPU_WINDOW", "KGPU_WINDOW_TEAM", "KGPU_WINDOW_FIRST"):
        monkeypatch.delenv(name, raising=False)
    if plan in TILE_PLANS:
        for name, v in TILE_PLANS[plan][0].items():
            monkeypatch.setenv(name, v)


def _check(tok, orc, plan, alone, batch, inside, monkeypatch, d, model):
    """every sentence of `alone` in a batch of its own, then `batch` in one; on the device-context plans the sentences for which `inside` holds must have
    been served by the pool kernel, the rest run with the windowed kernel behind it and must not reach the general kernel.  The redo and hand-on counts
    are the reservation model's (tests/pool_model.py), exactly: `tok` is a fresh handle, every batch on it steps the estimate by the restated rule of
    chain_feedback (M.steer: a batch of one sentence without a redo takes 1/128 off), and every batch runs on a context of its own, so the shipped plan's
    pool keeps its 40 KB shape (test_gpu_tile_groups.MODEL_PLANS)."""
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
        prof = _run(tok, orc, [s])
        want = predicted([s], est)
        assert sum(prof["deferred"]) == 0 and want[0] == 0, (s, prof)   # the pool kernel served it
        assert prof["redone"][0] == want[1], (s, want, prof)
        est = M.steer(est, want[1], 1)
    ins = [s for s in batch if inside(s)]
    beyond = [s for s in batch if not inside(s)]
    prof = _run(tok, orc, ins)
    want = predicted(ins, est)
    print(f"{plan}: {len(ins)} sentences meant for the pool kernel: deferred {prof['deferred']} redone {prof['redone']} (est_q8 {est}); {len(beyond)} beyond")
    assert sum(prof["deferred"]) == 0 and want[0] == 0 and prof["redone"][0] == want[1], (want, prof)
    if beyond:
        monkeypatch.setenv("KGPU_WINDOW", "24")
        tok2 = Tokenizer(d)
        try:
            prof = _run(tok2, orc, beyond)
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
    assert all(_need(pyref, pd, b * (SHIPPED_CHARS // len(b))) * 6 <= 32 * 624 * 5 for b in BASES)
    assert all(_need(pyref, pd, b * 12 + "あ") * 6 <= 64 * 2544 * 5 for b in BASES)
    inside = (lambda s: len(s) <= SHIPPED_CHARS) if limit == 32 * 624 else (lambda s: True)
    _set_plan(monkeypatch, plan)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    try:
        _check(tok, orc, plan, BASES, _sentences(np.random.default_rng(k)), inside, monkeypatch, d, _model(k))
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
    batch = _sentences(rng) + DEAD_ENDS + BEHIND_TE + [a + b for a in BEHIND_TE for b in DEAD_ENDS[:4]]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    inside = (lambda s: len(s) <= SHIPPED_CHARS) if plan == "shipped" else (lambda s: True)
    try:
        _check(tok, orc, plan, BASES + DEAD_ENDS + BEHIND_TE, batch, inside, monkeypatch, d, _model(k, True))
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
            prof = _run(tok, orc, ["あいう" * 40, "あいう", ("テ" if negative else "") + "あいういう" * 24, "いあいう" * 3, ""])
            print(f"k={k} {plan} negative={negative}: deferred {prof['deferred']} redone {prof['redone']} long_launches {prof['long_launches']}")
        finally:
            tok.close()
