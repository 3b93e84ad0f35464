"""The pool kernel's front end after its diet (kanpyo_amd/csrc/kgpu_pool.hip: the window decode of phase 0b, the attempt loop that no longer sees B and
C as invariants, the one-loop tile-list builder 3c, the token search that skips its two widest steps below 64 characters), at the sizes where that
code takes another path.  Every batch is the oracle's bit for bit (kernel_run.device_batch) and `deferred`, `redone`, `window_handed`, `tail_reruns`
(with `window_reruns` and `arena_regrows`) EQUAL what tests/pool_model.py predicts from the lattice's shape (kernel_run.run_case): nothing a
sentence decides may have changed.

round edges   C = 1, 2, 61, 62, 63, 64, 65, 126, 127 characters, once of one byte and once of three: the lane = position loops (decode, walk, scan, emit,
              3c) go from one round to two at C = 64 / C + 2 = 64 and to three behind 126; below 64 the token search starts at the step of 32.
alignment     the sentence's first byte at alignments 0..3 of the text, B + alignment + 4 = 255, 256, 257: the one-load edge, and every phase of the
              decode window's byte-align (three-byte characters at every offset of a dword).
positions     no prefix, one, a surface of 7 and of 8 records (the record count that the parked match cannot hold is looked up), a position nothing
              starts at, a sentence without any tile.  Eight and nine prefixes at a position and the unknown rider behind seven and eight are
              tests/pool_cases.py's cases e and f (test_gpu_pool_limits.py runs them).
tile list     positions of 1, 2, 4 and 6 tiles in one sentence, T and P up to 17; the device lattice (kgpu_lattice_dump) has the shape the model counted.
tickets       8 200 two-character sentences in one batch -- more than two per wavefront of the full grid, so a ticket beyond the workgroup's first round
              takes the division -- alone, and behind a batch that armed the second pool, whose launch takes its sentences from a work list.

Not here: a packed scan's field limits -- that cut was measured on the listing and not kept (profiles/experiments/pool_front_diet.txt)."""
import functools

import numpy as np
import pytest

import pool_cases as PC
import pool_model as M
from kernel_run import COUNTERS, libs, run_case, run_fresh, set_env  # noqa: F401  (libs: the fixture)
from window_cases import make_parts

pytestmark = pytest.mark.gpu

ROUND_EDGES = [1, 2, 61, 62, 63, 64, 65, 126, 127]
ENV_160 = {"KGPU_WINDOW_FIRST": "0"}   # (a batch's average length must not send it to the windowed kernel first)


@functools.lru_cache(maxsize=None)
def dict_mixed():
    """one-byte and three-byte keys, a dense surface ("あ" x 9: two target groups) and two-character keys across them"""
    return PC.Dictionary(make_parts([("a", 1), ("ab", 2), ("b", 1), ("あ", 9), ("い", 1), ("あい", 2)], seed=31))


@functools.lru_cache(maxsize=None)
def dict_records():
    """surfaces of 7 and of 8 records (3 bits hold 1..7: the eighth is looked up), one of 1, and NO unknown word for the default category: nothing
    starts at a katakana or an ASCII character"""
    return PC.Dictionary(make_parts([("あ", 7), ("い", 8), ("う", 1), ("あい", 1)], unk=(0, 1, 1), seed=41))


@functools.lru_cache(maxsize=None)
def dict_tiles():
    """record counts 1, 9 and 17 on single characters: (T, P) of a position is (its own count, its predecessor's)"""
    return PC.Dictionary(make_parts([("う", 1), ("え", 9), ("お", 9), ("あ", 17), ("い", 9)], seed=51))


def edge_sentences():
    out = []
    for c in ROUND_EDGES:
        out.append(("ab" * 64)[:c])        # one byte a character
        out.append(("あい" * 64)[:c])      # three bytes a character
    return out


# ------------------------------------------------------------------------------------------------------------------------------------- round edges
@pytest.mark.parametrize("plan", [M.PLAN_160, M.PLAN_SHIPPED], ids=["160x4", "shipped"])
def test_round_edges(libs, plan, monkeypatch):
    d = dict_mixed()
    sents = edge_sentences()
    verdicts = {s: d.verdict(s, plan)["verdict"] for s in sents}
    if plan == M.PLAN_160:
        assert all(v in (M.HELD, M.REDONE) for v in verdicts.values()), verdicts   # the pool kernel serves every length itself
    else:
        # the shipped pool routes the longest ones before the walk: what it serves itself is asserted, the others stay out of the batch (the windowed
        # kernel's own limits are tests/test_gpu_window_limits.py's)
        sents = [s for s in sents if verdicts[s] in (M.HELD, M.REDONE)]
        assert {len(s) for s in sents} >= {1, 2, 61, 62, 63, 64, 65}, sorted({len(s) for s in sents})
    # every sentence alone is too many handles: the edges in one batch among short ones, then the two-round and three-round ones on their own
    batches = [PC.Batch(d, plan, PC.among(sents, k=2), "all edges"), PC.Batch(d, plan, [s for s in sents if len(s) >= 62], "62 and more, alone")]
    run_case(PC.Case("round edges", d, plan, batches, env=ENV_160 if plan == M.PLAN_160 else None), libs[1], monkeypatch)


# --------------------------------------------------------------------------------------------------------------------------------------- alignment
def _of_bytes(nbytes, three):
    """a sentence of exactly `nbytes` bytes: `three` three-byte characters spread among one-byte ones, so that lead bytes meet every offset of a dword"""
    ones = nbytes - 3 * three
    assert ones >= three
    gap, s = ones // three, ""
    for i in range(three):
        s += ("ab" * 64)[:gap + (1 if i < ones % three else 0)] + "あい"[i % 2]
    assert len(s.encode()) == nbytes
    return s


def aligned_batch(tsh, three):
    """sentences of B = 251 - tsh, 252 - tsh, 253 - tsh bytes (B + tsh + 4 = 255, 256, 257) with `three` three-byte characters, each starting at
    alignment tsh of the packed text: short pad sentences in front of them bring the running offset there"""
    out, at = [], 0
    for total in (255, 256, 257):
        pad = (tsh - at) % 4
        out.append("a" * pad)
        at += pad
        s = _of_bytes(total - 4 - tsh, three)
        assert at % 4 == tsh
        out.append(s)
        at += len(s.encode())
    return out


@pytest.mark.parametrize("tsh", [0, 1, 2, 3])
def test_one_load_edge_at_every_alignment(libs, tsh, monkeypatch):
    import torch

    # (the packed text goes to the device as one tensor: its base is aligned far beyond a dword, so a sentence's alignment is its offset's)
    assert torch.empty(1000, dtype=torch.uint8, device="cuda:0").data_ptr() % 256 == 0
    d, plan = dict_mixed(), M.PLAN_SHIPPED
    batches = []
    # mostly one-byte characters: the match buffer is the peak and the first reservation too small -- every sentence is redone, the one-load ones staging
    # their text from the register first and the long way on the redo; mostly three-byte ones: held at the first attempt
    for three, want in ((11, M.REDONE), (60, M.HELD)):
        sents = aligned_batch(tsh, three)
        targets = [s for s in sents if len(s) > 4]
        assert [d.verdict(s, plan)["one_load"][tsh] for s in targets] == [True, True, False]   # 255 and 256 are one load, 257 stages the long way
        assert [d.verdict(s, plan)["verdict"] for s in targets] == [want] * 3
        batches.append(PC.Batch(d, plan, sents, f"255, 256, 257 with {three} three-byte characters"))
    run_case(PC.Case(f"alignment {tsh}", d, plan, batches), libs[1], monkeypatch)


# --------------------------------------------------------------------------------------------------------------------------------------- positions
def test_prefix_and_record_counts(libs, monkeypatch):
    d, plan = dict_records(), M.PLAN_SHIPPED
    look = lambda s: d.look(s)[2]   # (T, P) per start position
    assert look("あ") == [(7, 1), (1, 7)] and look("い") == [(8, 1), (1, 8)]   # a surface of 7 records, one of 8
    sents = ["あ", "い", "う", "あい", "あいう", "いあい", "ん", "んあ", "テ", "テあ", "あテい", "x", "xい", "", "ういあ" * 9, "テテ"]
    # what the cases are, by the shape model: a surface of 7 and of 8 records; no prefix but an unknown word ("ん"); nothing at all starts at "テ" / "x"
    pre = lambda s: d.look(s)[3]
    assert pre("あ") == [[1]] and pre("あい")[0] == [1, 2] and pre("ん") == [[]] and pre("テ") == [[]]
    assert look("ん")[0] == (1, 1) and look("テ")[0] == (0, 1) and look("テ")[1] == (1, 0)   # "テ": nothing starts at 0, EOS is dead: no tile at all
    assert sum(M.tile_count(t, p) for t, p in look("テ")) == 0 and sum(M.tile_count(t, p) for t, p in look("テテ")) == 0
    assert look("あテい") == [(7, 1), (0, 7), (8, 0), (1, 8)]   # a position nothing starts at inside a sentence, and a dead one behind it
    run_case(PC.Case("positions", d, plan, [PC.Batch(d, plan, sents, "all"), PC.Batch(d, plan, ["テ"], "no tile, alone"), PC.Batch(d, plan, ["い" * 20], "8 records x 20")]),
             libs[1], monkeypatch)


# --------------------------------------------------------------------------------------------------------------------------------------- tile list
def test_tile_list_of_1_2_4_6(libs, monkeypatch):
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.lattice import dump_lattice

    d, plan = dict_tiles(), M.PLAN_SHIPPED
    s = "うえおあいう"
    tp = d.look(s)[2]
    assert tp == [(1, 1), (9, 1), (9, 9), (17, 9), (9, 17), (1, 9), (1, 1)], tp
    assert [M.tile_count(t, p) for t, p in tp] == [1, 2, 4, 6, 6, 2, 1]
    sents = [s, s * 2, "あ" + s, s + "あ", "あああ", "いあ" * 4, s[::-1]]
    run_case(PC.Case("tile list", d, plan, [PC.Batch(d, plan, PC.among(sents, k=1), "among short ones"), PC.Batch(d, plan, [s], "alone")]), libs[1], monkeypatch)
    # the device's own lattice of s has the shape the model counted: nodes per start position, entries per bucket
    set_env(monkeypatch, {})
    tok = Tokenizer(Dict.from_parts(**d.parts))
    try:
        lat = dump_lattice(tok, s)
    finally:
        tok.close()
    assert len(lat.nodes) == 1 + sum(t for t, _ in tp)
    assert [len(e) for e in lat.edges[:len(s) + 1]] == [p for _, p in tp]
    starts = [0] * (len(s) + 1)
    for n in lat.nodes[1:]:
        starts[n.char_pos] += 1
    assert starts == [t for t, _ in tp]


# ----------------------------------------------------------------------------------------------------------------------------------------- tickets
@functools.lru_cache(maxsize=None)
def many_short(n=8200, seed=7):
    rng = np.random.default_rng(seed)
    abc = list("あいabうテ")
    return ["".join(rng.choice(abc, size=2)) for _ in range(n)]


def test_tickets_beyond_the_first_round(libs, monkeypatch):
    """more than two sentences for every wavefront the full grid has (1024 workgroups of four on the shipped pool): tickets W and up take the division"""
    d, plan = dict_mixed(), M.PLAN_SHIPPED
    b = PC.Batch(d, plan, many_short(), "8200 x two characters")
    assert set(b.labels) == {M.HELD}
    run_case(PC.Case("tickets", d, plan, [b]), libs[1], monkeypatch)


def test_tickets_from_a_work_list(libs, monkeypatch):
    """Two pools ("40:4:32,160:4").  The first batch leaves the first pool sentences, which arms the second (kgpu_chain.cpp: big_pool_batches); in the next
    batch the second pool's launch reads its work from the first one's list (WorkIO::in_list) -- the 8 200 short sentences with three long ones the
    first pool routes before the walk and the second holds."""
    from kanpyo_amd import Dict, Tokenizer

    d = dict_mixed()
    long3 = ["い" * 110, "い" * 120, "ab" * 100 + "い" * 60]
    est0 = M.EST_Q8_FRESH
    first = PC.SHORT + long3
    v_first = [d.verdict(s, M.PLAN_SHIPPED, est0)["verdict"] for s in first]
    assert [v for v in v_first if v != M.HELD] == [M.ROUTED_BEFORE_WALK] * 3
    est1 = M.steer(est0, 0, len(first))
    second = many_short() + long3
    v0 = [d.verdict(s, M.PLAN_SHIPPED, est1)["verdict"] for s in second]
    assert M.counters(v0) == (3, 0)
    assert all(d.verdict(s, M.PLAN_160, est1)["verdict"] == M.HELD for s in long3)   # ... and the 160 KB pool holds the three without a redo
    set_env(monkeypatch, {"KGPU_POOL": "40:4:32,160:4"})
    dd = Dict.from_parts(**d.parts)
    orc = libs[1].OracleTokenizer.from_dict(dd)
    tok = Tokenizer(dd)
    try:
        p1 = run_fresh(tok, orc, first)
        assert p1["deferred"][0] == 3 and p1["redone"] == [0, 0, 0, 0], p1   # (one pool in this chain: the windowed kernel served the three)
        p2 = run_fresh(tok, orc, second)
        got = {k: p2[k] for k in COUNTERS}
        print(f"work list: first {p1['deferred']} second {got}")
        assert got == {"deferred": [3, 0, 0, 0], "redone": [0, 0, 0, 0], "window_handed": [0] * 10, "tail_reruns": 0, "window_reruns": 0, "arena_regrows": 0}, got
    finally:
        tok.close()
