"""The pool kernel's front end (kanpyo_amd/csrc/kgpu_pool.hip: reserve, redo, hand on), each decision met at its edge with the routing counters asserted
as EXACT numbers.

The chain behind the pool kernel makes the tokens right whichever kernel served a sentence, so tokens alone cannot show a pool kernel that hands on too
much or too little, or a redo that quietly became a hand-on.  For a fresh dictionary handle and one batch, what the kernel decides about a sentence is a
function of that sentence alone; tests/pool_model.py restates that arithmetic line by line, tests/pool_cases.py chooses dictionaries and sentences with
it -- a HELD sentence just inside each limit, a REDONE or handed one just outside -- and tests/test_pool_model_cpu.py asserts every such claim without
a device.  Here every batch runs on a FRESH Tokenizer (Steering::est_q8 is the initial 64 x 256) with KGPU_POOL set explicitly ("40:4:32": the shipped
shape without the per-batch choices of the shipped plan; "160:4" with KGPU_WINDOW_FIRST=0); records, offsets and status are the oracle's bit for bit
(kernel_run.device_batch) and deferred, redone, window_handed, tail_reruns, window_reruns and arena_regrows EQUAL the model's prediction:

a  routed before the walk at the exact page (n = 100 / 101 x "あ", 32 / 33 pages);
b  the redo from both sides of a page -- need_full binding, need_emit binding, and a one-load sentence whose redo stages the text the long way --
   and a mixed batch of 200 with its redo count;
c  routed after the walk (first reservation within max_pages, exact need beyond), its neighbour redone and held;
d  64 identical sentences that all redo, two at a time per pool: the designed wait of the deadlock rule;
e  MAXM: eight prefixes at a position held, nine handed on and held by the windowed kernel;
f  the unknown word's rider with 7 / 8 prefixes in front of it and 7 / 8 / 9 unknown records;
g  the 8-bit length: a key of 255 characters held, one of 256 handed on by the pool and by the windowed kernel (window_handed[2]);
h  the small call's one-wavefront slice: the exact need just inside and just outside 65 024 bytes (small_fallbacks);
i  the estimate learns: the mixed batch three times on ONE handle, the redo count following the restated steering step.

Left out on purpose: `N > 0xFFFF || Nb + 1 > SLOT_MAX` cannot be reached (neither fits a pool of 160 KB); the pool_wait_alloc time-out is not to be
provoked; the one-load byte lengths and alignments are test_byte_length_and_alignment_boundaries', the WIDE layout is test_plain_leaves_layout's."""
import pytest

import pool_cases as PC
from kernel_run import COUNTERS, host_batch, libs, run_case, run_fresh, set_env  # noqa: F401  (libs: the fixture)

pytestmark = pytest.mark.gpu


def test_a_routed_before_the_walk(libs, monkeypatch):
    run_case(PC.case_a(), libs[1], monkeypatch)


@pytest.mark.parametrize("way", ["full", "emit", "short"])
def test_b_redo_from_both_sides_of_a_page(libs, way, monkeypatch):
    run_case(PC.case_b_pairs()[way], libs[1], monkeypatch)


def test_b_mixed_batch_redo_count(libs, monkeypatch):
    run_case(PC.case_b_mixed(), libs[1], monkeypatch)


def test_c_routed_after_the_walk(libs, monkeypatch):
    run_case(PC.case_c(), libs[1], monkeypatch)


def test_d_every_wavefront_of_a_pool_redoes(libs, monkeypatch):
    run_case(PC.case_d(), libs[1], monkeypatch)


def test_e_maxm(libs, monkeypatch):
    run_case(PC.case_e(), libs[1], monkeypatch)


@pytest.mark.parametrize("case", PC.cases_f(), ids=lambda c: c.name[3:].replace(" ", "_").replace(",", ""))
def test_f_the_unknown_words_rider(libs, case, monkeypatch):
    run_case(case, libs[1], monkeypatch)


@pytest.mark.parametrize("case", PC.cases_g(), ids=["255", "256"])
def test_g_the_8_bit_length(libs, case, monkeypatch):
    run_case(case, libs[1], monkeypatch)


def test_h_the_small_calls_slice(libs, monkeypatch):
    """kgpu_tokenize_batch with one sentence: served in the one launch while its exact need fits the slice, redone on the general path (small_fallbacks)
    when it does not -- the oracle's records either way."""
    from kanpyo_amd import Dict, Tokenizer

    set_env(monkeypatch, {})
    h = PC.case_h()
    d = Dict.from_parts(**h["d"].parts)
    orc = libs[1].OracleTokenizer.from_dict(d)
    for key, fallbacks in (("held", 0), ("handed", 1)):
        tok = Tokenizer(d)
        try:
            host_batch(tok, orc, PC.SHORT[:2] + [h[key]] + PC.SHORT[2:], what=key)
            r = tok.routing()
        finally:
            tok.close()
        print(f"small call, {key} ({len(h[key])} characters): small_calls {r['small_calls']} small_fallbacks {r['small_fallbacks']} deferred {r['deferred']} redone {r['redone']}")
        assert r["small_calls"] == 1 and r["small_fallbacks"] == fallbacks, (key, r)
        if not fallbacks:   # the one launch served it: nothing left the pool kernel, no reservation to prove too small
            assert r["batches"] == 1 and r["deferred"] == [0] * 4 and r["redone"] == [0] * 4, r
        else:               # the slice proved too small after the walk (one late count, one deferral); then the general path ran the call again, whose
            # pool kernel (the shipped plan) routes the sentence before the walk (test_pool_model_cpu.py): one more deferral, no late count
            assert r["batches"] == 2 and r["deferred"] == [2, 0, 0, 0] and r["redone"] == [1, 0, 0, 0], r


def test_i_the_estimate_learns(libs, monkeypatch):
    """the mixed batch three times on ONE handle: chain_feedback steps Steering::est_q8 by the redo count, and the next run's count is the model's under
    the stepped estimate"""
    from kanpyo_amd import Dict, Tokenizer

    case = PC.case_b_mixed()
    set_env(monkeypatch, case.env)
    d = Dict.from_parts(**case.parts)
    orc = libs[1].OracleTokenizer.from_dict(d)
    tok = Tokenizer(d)
    try:
        for est, b in PC.learning_runs():
            prof = run_fresh(tok, orc, b.sentences)
            got, want = {k: prof[k] for k in COUNTERS}, b.expect()
            print(f"est_q8 {est}: {got}")
            assert got == want, (est, got, want)
    finally:
        tok.close()
