"""The pool kernel's backtrace over quads (kanpyo_amd/csrc/kgpu_pool.hip, phase 5; kgpu_backtrace_core.h): behind stage B every node's best predecessor
is doubled into its four nearest ancestors -- all 64 lanes, four nodes a lane and trip -- and one lane then follows the best path four nodes a round.  Here:
sentences whose path length K and node count N are known by construction, at the sizes where that code takes another turn:

  K = 0 (EOS dead), 1 .. 9     the chain ends at every offset of a quad, on both sides of a quad boundary
  K = 63, 64, 65, 128, 129     the token loop's rounds behind the chase, lane 63's successor
  K = C + 1                    single-character words, at C = 1 and at the longest such sentence the shipped plan holds (100 x "あ": pool_cases.case_a)
  N - 1 = 255, 256, 257        (and 511, 512, 513) the trips of the four-per-lane passes: 256 nodes a trip
  unknown words on the path, dead positions and unreachable live nodes off it (their "none" must not be followed), a path that ends in a dead node,
  a sentence that is redone (the passes run over the second attempt's arrays)

each alone in its batch and among short sentences; tokens bit for bit the oracle's and the routing counters the model's (tests/pool_model.py), as in
tests/test_gpu_pool_limits.py -- a fresh handle per batch -- so that the pool kernel, not the chain behind it, is what served them.  K and N are asserted
here from the oracle and the lattice's shape BEFORE the device is asked.  Then the same sentences through the small call (one wavefront a workgroup, its
own LDS slice), with KGPU_BYTE_TRIE (the kernel's other walker) and with PROFILE_WORK (its profiling instantiation, whose K counter is the oracle's)."""
import functools

import numpy as np
import pytest

import pool_cases as PC
import pool_model as M
from kernel_cases import BASES, BEHIND_TE, DEAD_ENDS, dead_parts
from kernel_run import COUNTERS, host_batch, libs, run_case, run_fresh, set_env  # noqa: F401  (libs: the fixture)

pytestmark = pytest.mark.gpu

ENV_160 = {"KGPU_WINDOW_FIRST": "0"}   # (as pool_cases.cases_g: the batch's average length must not send it to the windowed kernel first)


class Group:
    """a dictionary, a plan and special sentences with the K (tokens, EOS included) each must have; `nodes`: sentence -> N - 1 it must have"""

    def __init__(self, name, d, plan, k_of, env=None, nodes=None, unknown=(), verdicts=None):
        self.name, self.d, self.plan, self.k_of, self.env, self.nodes, self.unknown = name, d, plan, dict(k_of), dict(env or {}), dict(nodes or {}), list(unknown)
        self.verdicts = dict(verdicts or {})

    @property
    def specials(self):
        return list(self.k_of)

    def case(self, extra_env=None):
        """every special sentence among short ones, then each alone: one batch each on a fresh handle"""
        batches = [PC.Batch(self.d, self.plan, PC.among(self.specials), "among short ones")] + [PC.Batch(self.d, self.plan, [s], f"alone: {len(s)} characters") for s in self.specials]
        return PC.Case(self.name, self.d, self.plan, batches, env=dict(self.env, **(extra_env or {})))

    def check_claims(self, orc):
        """K from the oracle, N from the lattice's shape, the verdicts from the model: what the case is there for, before a GPU is touched"""
        from kanpyo_amd.tokenizer import pack_sentences

        utf8, offs = pack_sentences(self.specials)
        exp = orc.tokenize_batch(utf8, offs, 2)
        counts = np.diff(exp.offsets.astype(np.int64))
        assert [int(c) for c in counts] == [self.k_of[s] for s in self.specials], (self.name, list(counts))
        for s, n1 in self.nodes.items():
            assert sum(t for t, _ in self.d.look(s)[2]) == n1, (self.name, len(s))   # N - 1: every node but BOS (EOS is position C's one target)
        cls = exp.tokens.view(np.int32).reshape(-1, 6)[:, 1]
        for s in self.unknown:
            i = self.specials.index(s)
            assert (cls[int(exp.offsets[i]):int(exp.offsets[i + 1])] == 2).any(), (self.name, s)   # KGPU_CLASS_UNKNOWN on the path
        for s in self.specials:
            v = self.d.verdict(s, self.plan)["verdict"]
            assert v == self.verdicts.get(s, M.HELD), (self.name, len(s), v)


@functools.lru_cache(maxsize=None)
def group_short():
    """dict_one ("あ", one record; one unknown record on whatever else): n x "あ" is n single-character words and EOS, K = n + 1 = C + 1"""
    d = PC.dict_one()
    k_of = {"あ" * n: n + 1 for n in list(range(0, 9)) + [62, 63, 64, 100]}
    k_of.update({"あxyzあ": 6, "xあ": 3, "あああx": 5})   # unknown single characters on the path (DEFAULT does not group)
    return Group("quads: K = 1 .. 9, 63 .. 65, C + 1 = 101", d, M.PLAN_SHIPPED, k_of, unknown=["あxyzあ", "xあ", "あああx"])


@functools.lru_cache(maxsize=None)
def group_long():
    d = PC.dict_one()
    return Group("quads: K = 128, 129", d, M.PLAN_160, {"あ" * 127: 128, "あ" * 128: 129}, env=ENV_160)


@functools.lru_cache(maxsize=None)
def group_trips():
    """dict_dense (nine records on "あ", one on "い"): "あ"^p "い"^q has 9 p + q + 1 nodes behind BOS; and the redo's two sentences (case b, "short" and
    "full": the first reservation proves too small after the scan, the passes run in the second attempt's carve)"""
    d = PC.dict_dense()
    nodes = {"あ" * 28 + "い" * q: 9 * 28 + q + 1 for q in (2, 3, 4)}
    nodes.update({"あ" * 56 + "い" * q: 9 * 56 + q + 1 for q in (6, 7, 8)})
    assert sorted(nodes.values()) == [255, 256, 257, 511, 512, 513]
    k_of = {s: len(s) + 1 for s in nodes}
    verdicts = {s: d.verdict(s, M.PLAN_SHIPPED)["verdict"] for s in nodes}
    assert set(verdicts.values()) <= {M.HELD, M.REDONE}   # served by the pool kernel either way
    for way in ("short", "full"):
        s = PC.case_b_pairs()[way].facts["redone"]
        k_of[s], verdicts[s] = len(s) + 1, M.REDONE
    return Group("quads: trips of 256 nodes, the redo", d, M.PLAN_SHIPPED, k_of, nodes=nodes, verdicts=verdicts)


@functools.lru_cache(maxsize=None)
def group_dead(negative):
    """test_gpu_dead_positions' dictionaries.  Plain: "あいう" has a dead position (k + 1 nodes without a predecessor) off the best path.  Negative costs:
    behind "テ" every node is unreachable, a dead node wins as a predecessor and the path ends in it (K counts from the middle of the sentence), or EOS
    itself is dead: K = 0."""
    d = PC.Dictionary(dead_parts(9, negative))
    sents = BASES + (DEAD_ENDS + BEHIND_TE if negative else ["あいう" * 7, "いあいう" * 5])
    from oracle import pyref

    from kanpyo_amd import Dict

    dd = Dict.from_parts(**d.parts)
    pd = pyref.PyDict(dd.index_dict, dd.connection_dict, dd.morph_dict, dd.unk_dict, dd.char_category, dd.invoke_list, dd.group_list)
    k_of = {s: len(pyref.tokenize(pd, s)) for s in sents}
    if negative:
        assert k_of["テ"] == 0 and k_of["テあ"] == 0 and k_of["テいう"] == 2 and {0, 2, 3, 4} <= set(k_of.values()), k_of
    else:
        assert min(k_of.values()) >= 2, k_of
    return Group(f"quads: dead positions{', negative costs' if negative else ''}", d, M.PLAN_SHIPPED, k_of)


GROUPS = {"short": group_short, "long": group_long, "trips": group_trips, "dead": lambda: group_dead(False), "dead_negative": lambda: group_dead(True)}


def _orc(libs, g):
    from kanpyo_amd import Dict

    d = Dict.from_parts(**g.d.parts)
    return d, libs[1].OracleTokenizer.from_dict(d)


@pytest.mark.parametrize("name", list(GROUPS))
def test_quads_alone_and_among_short_ones(libs, name, monkeypatch):
    g = GROUPS[name]()
    g.check_claims(_orc(libs, g)[1])
    run_case(g.case(), libs[1], monkeypatch)


@pytest.mark.parametrize("name", list(GROUPS))
def test_quads_byte_trie(libs, name, monkeypatch):
    """the kernel's byte-level walker (another instantiation of the same kernel)"""
    g = GROUPS[name]()
    monkeypatch.setenv("KGPU_BYTE_TRIE", "1")
    case = g.case()
    case.batches = case.batches[:1]
    run_case(case, libs[1], monkeypatch)


@pytest.mark.parametrize("name", list(GROUPS))
def test_quads_small_call(libs, name, monkeypatch):
    """kgpu_tokenize_batch with at most 128 sentences: one launch, one wavefront a workgroup with a slice of its own -- every special sentence alone, then all
    among short ones; nothing falls back to the general path (every one of them fits the slice of 65 024 bytes)"""
    from kanpyo_amd import Tokenizer

    g = GROUPS[name]()
    set_env(monkeypatch, {})
    d, orc = _orc(libs, g)
    assert all(g.d.verdict(s, M.PLAN_SMALL)["verdict"] == M.HELD for s in g.specials)
    tok = Tokenizer(d)
    try:
        batches = [[s] for s in g.specials] + [PC.among(g.specials)]
        for part in batches:
            assert len(part) <= 128 and sum(len(s.encode()) for s in part) < 16 * 1024
            host_batch(tok, orc, part, what=f"{g.name} {[len(s) for s in part]}")
        r = tok.routing()
        print(f"{g.name}: small_calls {r['small_calls']} small_fallbacks {r['small_fallbacks']}")
        assert r["small_calls"] == len(batches) and r["small_fallbacks"] == 0, r
    finally:
        tok.close()


@pytest.mark.parametrize("name", list(GROUPS))
def test_quads_profile_work(libs, name, monkeypatch):
    """the kernel's profiling instantiation: the same tokens, and its work counters -- K among them -- are the oracle's"""
    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import PROFILE_WORK
    from kanpyo_amd.tokenizer import pack_sentences

    g = GROUPS[name]()
    set_env(monkeypatch, dict({"KGPU_POOL": M.POOL_ENV[g.plan]}, **g.env))
    d, orc = _orc(libs, g)
    sentences = PC.among(g.specials)
    exp = orc.tokenize_batch(*pack_sentences(sentences), 2)
    tok = Tokenizer(d)
    try:
        prof, work = run_fresh(tok, orc, sentences, PROFILE_WORK, exp=exp, also=("work",))
        assert work == exp.counters, (work, exp.counters)
        want = PC.Batch(g.d, g.plan, sentences).expect()
        assert {k: prof[k] for k in COUNTERS} == want, (prof, want)
    finally:
        tok.close()
