"""Dictionaries and sentences CHOSEN AGAINST the pool kernel's front end (kanpyo_amd/csrc/kgpu_pool.hip: reserve, redo, hand on), shared by
tests/test_pool_model_cpu.py (which asserts every claim made here by the model and the naive lattice alone) and tests/test_gpu_pool_limits.py (which
asks the device for the same counters).  A case is a dictionary (Dict.from_parts arguments), a plan and batches of sentences; what each sentence's
verdict is, on which side of which boundary it lies and by how many bytes is said HERE, from tests/pool_model.py over the lattice's shape, before a
GPU is touched -- a change to a dictionary builder or to the kernel's arithmetic then cannot turn a case into a no-op.

The lattice's shape comes from the key list (window_cases.Shape: prefixes and unknown words per position, src/lattice.rs:42-99); the CPU
test checks it against oracle/pyref.py's naive lattice for every sentence used.  Nothing here needs a device or the library."""
import functools

import numpy as np

import pool_model as M
from window_cases import Shape, make_parts

SHORT = ["テスト", "", "漢字かな", "xyz テスト", "いうえお", "辞書x形態素"]   # ordinary company: a few characters each, HELD on every plan (asserted)


def tp_of(sh):
    """(T, P) per start position 0..C from a Shape: its nodes per position and EOS at C; what ends at each position and BOS at 0."""
    T = list(sh.per_pos) + [1]
    P = [0] * (sh.C + 1)
    P[0] = 1
    for _, e, _ in sh.entries():
        P[e] += 1
    return list(zip(T, P))


class Dictionary:
    """Dict.from_parts arguments with the model's view of a sentence over them (cached: the searches below ask often)."""

    def __init__(self, parts):
        self.parts = parts
        self._seen = {}

    def look(self, s):
        if s not in self._seen:
            sh = Shape(self.parts, s)
            self._seen[s] = (len(s.encode("utf-8")), sh.C, tp_of(sh), [[n for n, _ in p] for p in sh.prefixes])
        return self._seen[s]

    def verdict(self, s, plan, est_q8=M.EST_Q8_FRESH, **kw):
        B, C, tp, pre = self.look(s)
        return M.verdict(B, C, tp, plan, est_q8, prefix_chars=pre, **kw)


def margin(v):
    """Bytes between the sentence's exact need and its first reservation: >= 0 it fits (HELD), < 0 it does not."""
    return v["lds_bytes"] - max(v["need_emit"], v["need_full"])


class Batch:
    """Sentences for ONE batch on a fresh handle, and the counters the model expects of it."""

    def __init__(self, d, plan, sentences, note="", est_q8=M.EST_Q8_FRESH, window_handed=None):
        self.sentences, self.note, self.est_q8 = list(sentences), note, est_q8
        self.verdicts = [d.verdict(s, plan, est_q8) for s in self.sentences]
        self.labels = [v["verdict"] for v in self.verdicts]
        self.deferred0, self.redone0 = M.counters(self.labels)
        # what the windowed kernel behind the pool hands on in its turn (why code -> sentences): none unless the case says so
        self.window_handed = dict(window_handed or {})

    def expect(self):
        """The routing counters of the batch: deferred, redone, window_handed, tail_reruns, window_reruns, arena_regrows."""
        handed = sum(self.window_handed.values())
        return {"deferred": [self.deferred0, handed, 0, 0], "redone": [self.redone0, 0, 0, 0],
                "window_handed": [self.window_handed.get(i, 0) for i in range(10)],
                # a fresh handle's chain ends on the windowed kernel (Steering::tail_batches starts at 0, kgpu_chain.h:89): what that one hands on is a tail pass
                "tail_reruns": 1 if handed else 0, "window_reruns": 0, "arena_regrows": 0}


class Case:
    def __init__(self, name, d, plan, batches, env=None, facts=None):
        self.name, self.d, self.plan, self.batches, self.facts = name, d, plan, batches, dict(facts or {})
        self.env = {"KGPU_POOL": M.POOL_ENV[plan]}
        self.env.update(env or {})

    @property
    def parts(self):
        return self.d.parts


def among(special, k=3):
    """the special sentences between ordinary ones"""
    out = list(SHORT[:k])
    for i, s in enumerate(special):
        out += [s] + SHORT[(i + k) % len(SHORT):][:2]
    return out + SHORT


def step_pair(d, plan, family, want, est_q8=M.EST_Q8_FRESH):
    """The first (shorter, longer) of `family` -- pairs of sentences one character apart -- whose shorter one is HELD, whose longer one is REDONE and
    for which want(verdict of shorter, verdict of longer) holds."""
    for a, b in family:
        va, vb = d.verdict(a, plan, est_q8), d.verdict(b, plan, est_q8)
        if va["verdict"] == M.HELD and vb["verdict"] == M.REDONE and want(va, vb):
            return a, b
    raise AssertionError("no such pair in the family")


# ------------------------------------------------------------------------------------------------------------------------------------ the dictionaries
@functools.lru_cache(maxsize=None)
def dict_one():
    """k = 1 record on "あ": a sparse lattice (about 55 bytes of LDS a character against the estimate's 192)."""
    return Dictionary(make_parts([("あ", 1)], seed=21))


@functools.lru_cache(maxsize=None)
def dict_dense(k=9):
    """k records on "あ", one on "い": 12 k bytes of nodes, 8 k of bucket entries and 8 ceil(k / 8)^2 of tiles a character "あ" -- with k = 9 about 241
    bytes a character against the estimate's 192, so the first reservation proves too small once the sentence is long enough."""
    return Dictionary(make_parts([("あ", k), ("い", 1)], seed=22))


@functools.lru_cache(maxsize=None)
def dict_ascii():
    """One record on "a": one node a character of ONE byte -- 27 bytes of per-character arrays, 12 of node and 32 of parked matches against 8 of bucket
    entry and 8 of tile: the match buffer, not the sweep, is the peak (need_emit > need_full), at 71 bytes a byte against the estimate's 64."""
    return Dictionary(make_parts([("a", 1)], seed=23))


@functools.lru_cache(maxsize=None)
def dict_nested(deepest, unk_hiragana=1, invoke_hiragana=0):
    """Keys "あ"^1 .. "あ"^deepest, one record each: min(deepest, what is left) prefixes at every position of a run of "あ"."""
    parts = make_parts([("あ" * n, 1) for n in range(1, deepest + 1)], invoke=(0, 1, invoke_hiragana), unk=(1, 1, unk_hiragana), seed=24 + deepest)
    if invoke_hiragana:
        # the unknown records compete with the keys (make_parts prices them out: 3000-6000 against -500-5000), so the best path takes some
        parts["unk_morphs"] = [[l, r, c - 4500] for l, r, c in parts["unk_morphs"]]
    return Dictionary(parts)


@functools.lru_cache(maxsize=None)
def dict_long_key(chars):
    """One key of `chars` x "あ" (and "い"): a match whose length is `chars` characters."""
    return Dictionary(make_parts([("あ" * chars, 1), ("い", 1)], seed=25))


# ------------------------------------------------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def case_a():
    """Routed before the walk, at the exact page: est = 192 n + 768 for n x "あ" on 40:4:32 -- n = 100 is 19 968 bytes = 32 pages, n = 101 is 33."""
    d, plan = dict_one(), M.PLAN_SHIPPED
    held, routed = "あ" * 100, "あ" * 101
    return Case("a: routed before the walk", d, plan,
                [Batch(d, plan, among([held, routed]), "both among short ones"), Batch(d, plan, [held], "100 alone"), Batch(d, plan, [routed], "101 alone")],
                facts={"held": held, "routed": routed})


def _family_dense(lo, hi):
    """pairs "あ"^p "い"^q / "あ"^(p + 1) "い"^q with lo <= p + q and p + q + 1 <= hi characters"""
    for q in range(0, 64):
        for p in range(max(1, lo - q), hi - q):
            yield "あ" * p + "い" * q, "あ" * (p + 1) + "い" * q


@functools.lru_cache(maxsize=None)
def case_b_pairs():
    """The redo from both sides of a page, three ways (-> {way: (case, held, redone)}):
    full   need_full is what does not fit (need_emit does), both sentences of 253 bytes or more: every attempt stages the text the long way;
    emit   need_emit is what does not fit (need_full does);
    short  a sentence of at most 249 bytes whatever its alignment: the first attempt stages it from the one-load register, the redo the long way."""
    plan, out = M.PLAN_SHIPPED, {}
    long_way = lambda v: not any(v["one_load"])
    one_load = lambda v: all(v["one_load"])
    d = dict_dense()
    ways = {
        "full": (d, _family_dense(85, 87), lambda a, b: long_way(a) and long_way(b) and b["need_full"] > b["lds_bytes"] >= b["need_emit"]),
        "short": (d, _family_dense(1, 83), lambda a, b: one_load(a) and one_load(b) and b["need_full"] > b["lds_bytes"] >= b["need_emit"]),
        "emit": (dict_ascii(), (("a" * p + "x" * q, "a" * (p + 1) + "x" * q) for q in (0, 5, 17) for p in range(96, 240)),
                 lambda a, b: b["need_emit"] > b["lds_bytes"] >= b["need_full"]),
    }
    for way, (dd, family, want) in ways.items():
        held, redone = step_pair(dd, plan, family, want)
        case = Case(f"b: the redo, {way}", dd, plan,
                    [Batch(dd, plan, among([held, redone]), "both among short ones"), Batch(dd, plan, [held], "held alone"), Batch(dd, plan, [redone], "redone alone")],
                    facts={"held": held, "redone": redone})
        out[way] = case
    return out


@functools.lru_cache(maxsize=None)
def mixed_sentences(n=200, seed=5):
    """about 200 sentences "あ"^p "い"^q over dict_dense: some dense enough for a redo, some not, none anywhere near the routing limit"""
    rng = np.random.default_rng(seed)
    return ["あ" * int(rng.integers(0, 41)) + "い" * int(rng.integers(0, 21)) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def case_b_mixed():
    d, plan = dict_dense(), M.PLAN_SHIPPED
    return Case("b: a mixed batch", d, plan, [Batch(d, plan, mixed_sentences(), "200 sentences")])


@functools.lru_cache(maxsize=None)
def learning_runs(runs=3):
    """(i) the mixed batch `runs` times on ONE handle -> [(est_q8 the run starts with, Batch)]: the estimate stepped by the restated rule after each."""
    d, plan, est, out = dict_dense(), M.PLAN_SHIPPED, M.EST_Q8_FRESH, []
    sents = mixed_sentences()
    for _ in range(runs):
        b = Batch(d, plan, sents, f"est_q8 {est}", est_q8=est)
        out.append((est, b))
        est = M.steer(est, b.redone0, len(sents))
    return out


@functools.lru_cache(maxsize=None)
def case_c():
    """Routed after the walk: the first reservation is within max_pages, the exact need beyond; the neighbour one "あ" shorter is redone and held."""
    d, plan = dict_dense(), M.PLAN_SHIPPED
    p = next(p for p in range(2, 101) if d.verdict("あ" * p, plan)["verdict"] == M.ROUTED_AFTER_WALK)
    routed, redone = "あ" * p, "あ" * (p - 1)
    return Case("c: routed after the walk", d, plan,
                [Batch(d, plan, among([redone, routed]), "both among short ones"), Batch(d, plan, [routed], "routed alone"), Batch(d, plan, [redone], "redone alone")],
                facts={"routed": routed, "redone": redone})


@functools.lru_cache(maxsize=None)
def case_d():
    """64 identical sentences whose exact need is 30 to 32 pages and whose first reservation is smaller: 16 workgroups of four wavefronts that all redo,
    two at a time per pool."""
    d, plan = dict_dense(), M.PLAN_SHIPPED
    p = next(p for p in range(2, 101) if d.verdict("あ" * p, plan)["verdict"] == M.REDONE and d.verdict("あ" * p, plan)["npg_redo"] >= 30)
    return Case("d: every wavefront redoes", d, plan, [Batch(d, plan, ["あ" * p] * 64, "64 identical")], facts={"sentence": "あ" * p})


@functools.lru_cache(maxsize=None)
def case_e():
    """MAXM: nested keys "あ"^1 .. "あ"^9 -- "あ" x 8 has eight prefixes at position 0 (held), "あ" x 9 nine (handed on; the windowed kernel parks the ninth)."""
    d, plan = dict_nested(9), M.PLAN_SHIPPED
    held, handed = "あ" * 8, "あ" * 9
    return Case("e: MAXM", d, plan,
                [Batch(d, plan, among([held]), "eight prefixes"), Batch(d, plan, among([handed]), "nine prefixes"), Batch(d, plan, among([held, handed, "x" + handed, held + "x"]), "both")],
                facts={"held": held, "handed": handed})


@functools.lru_cache(maxsize=None)
def cases_f():
    """The unknown word's rider: hiragana invokes unknown words with 7, 8 or 9 records; at a position with 7 dictionary prefixes the rider has slot 7 of the
    match buffer, with 8 it has none and emit 3a looks the category up (as it does for a count of 8 or 9, which the 3-bit field stores as 0)."""
    out = []
    for deepest in (7, 8):
        for unk in (7, 8, 9):
            d, plan = dict_nested(deepest, unk_hiragana=unk, invoke_hiragana=1), M.PLAN_SHIPPED
            sents = ["あ" * deepest, "あ" * (deepest + 5), "x" + "あ" * deepest + "テ", "あ" * (deepest - 1), "あ"]
            out.append(Case(f"f: {deepest} prefixes, {unk} unknown records", d, plan, [Batch(d, plan, among(sents), "")],
                            facts={"deepest": deepest, "unk": unk, "sentences": sents}))
    return out


@functools.lru_cache(maxsize=None)
def cases_g():
    """The 8-bit length, on 160:4: a key of 255 characters is parked and held, one of 256 is handed on -- and by the windowed kernel as well (why 2)."""
    plan, env = M.PLAN_160, {"KGPU_WINDOW_FIRST": "0"}
    d = dict_long_key(255)
    held = Case("g: a key of 255 characters", d, plan, [Batch(d, plan, among(["あ" * 255, "あ" * 256]), "")], env=env, facts={"sentences": ["あ" * 255, "あ" * 256]})
    d = dict_long_key(256)
    handed = Case("g: a key of 256 characters", d, plan, [Batch(d, plan, among(["あ" * 256]), "", window_handed={2: 1}), Batch(d, plan, among(["あ" * 255]), "no match")],
                  env=env, facts={"sentences": ["あ" * 256]})
    return [held, handed]


@functools.lru_cache(maxsize=None)
def case_h():
    """The small call's slice (one wavefront, 64 pages of 1016 bytes, no estimate): the longest "あ" x p over dict_dense whose exact need fits
    65 024 bytes, and one "あ" more."""
    d, plan = dict_dense(), M.PLAN_SMALL
    assert d.verdict("あ" * 256, plan)["verdict"] == M.HELD   # (about 241 bytes a character: the search starts well inside the slice)
    p = next(p for p in range(256, 400) if d.verdict("あ" * (p + 1), plan)["verdict"] != M.HELD)
    return {"d": d, "plan": plan, "held": "あ" * p, "handed": "あ" * (p + 1)}


@functools.lru_cache(maxsize=None)
def all_cases():
    return [case_a()] + list(case_b_pairs().values()) + [case_b_mixed(), case_c(), case_d(), case_e()] + cases_f() + cases_g()
