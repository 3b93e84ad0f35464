"""The windowed kernel's hand-on limits (kanpyo_amd/csrc/kgpu_window.hip), each reached on purpose and told apart by kgpu_routing.window_handed.

The kernel holds a sentence of any length in a bounded LDS; what it cannot hold it pushes onto the next launch's work list and counts under the
limit it ran into (`why`, codes 1-8, the table at kgpu_routing in include/kanpyo_gpu.h).  Every exit is a `break` out of a loop that holds LDS
state, prefetched registers and -- in the two-wavefront (TEAM) form -- two tokens another wavefront polls, so every case here is a PAIR on tiny
dictionaries (Dict.from_parts): a HELD sentence just inside the limit (nothing deferred, every counter 0) and a HANDED one just outside it (exactly
the intended counter, every other one 0), between ordinary sentences, bit-exact against the oracle (records, offsets, status: no tolerance), run
twice with identical routing.  KGPU_POOL=0: every sentence enters the windowed kernel, so deferred[0] is what it handed on; with
KGPU_WINDOW_TEAM=2 the team hands to list 0 and the ordinary form behind it to list 1 (a sentence neither holds is counted twice).

Which side of a limit a sentence is on is decided BEFORE the GPU is touched, from a plain-Python model of the lattice's shape (window_cases.Shape: the
nodes per start position from the key list, the category table and the unknown-word rules of src/lattice.rs:42-99) whose node total must equal the
oracle's (counters["N"]) for every sentence: tests/window_cases.py's scenarios_* functions, which tests/test_window_limits_cpu.py runs without a
device.  A change to a dictionary builder then cannot turn a case into a no-op.  The batches run through tests/kernel_run.py (run_batch, run_scenario).

Left out on purpose:
* sentences of 2^24 bytes or more and a refused launch configuration (cfg_bad): too large for a test / unreachable from a valid plan; both are
  handed on uncounted (window_handed[0] stays 0);
* `cbad` in the ordinary form (a carried node index below the next window's base): it needs more than 32768 nodes inside 64 positions, which the
  window's own N > 0x7FFF test catches first;
* the Control::window_fail -> kgpu_routing.window_reruns rerun on the host: build_chain and tail_chain give every Window step an output list, so
  the kernel's branch without one cannot run today (tests/c_abi/chain_policy.cpp checks that on every chain it builds).
"""
import numpy as np
import pytest

from kernel_run import libs, run_batch, run_scenario  # noqa: F401  (libs: the fixture)
from window_cases import (ORDINARY, arena_batches, scenarios_why1, scenarios_why2, scenarios_why3, scenarios_why4, scenarios_why6, scenarios_why7,
                          scenarios_why8)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("team", [False, True], ids=["ordinary", "team"])
@pytest.mark.parametrize("make", [scenarios_why1, scenarios_why2, scenarios_why4, scenarios_why6, scenarios_why8], ids=lambda f: f.__name__[10:])
def test_limit_held_and_handed(libs, make, team, monkeypatch):
    """whys 1, 2, 4, 6 and 8 in both forms: held -> nothing deferred, every counter 0; handed -> exactly the intended counter (twice per batch: the
    sentence is in it twice; in the team form once more by the ordinary form behind it), window_handed[8] and every other index 0.  (why 4 has a second held
    twin that the team hands to the ordinary form: scenarios_why4.)"""
    for sc in make():
        run_scenario(sc, team, monkeypatch)


def test_node_limit(libs, monkeypatch):
    """why 3: a sentence of 262143 nodes is held, one of 262144 is handed on -- by the ordinary form and by the team."""
    held, handed = scenarios_why3()
    run_scenario(held, False, monkeypatch)
    run_scenario(handed, False, monkeypatch)
    run_scenario(handed, True, monkeypatch)


def test_carry_banks_of_the_team_form(libs, monkeypatch):
    """why 7: 324 carried entries fit a bank, 456 and more do not: the team hands the sentence to the ordinary form, which holds it (deferred[1] == 0);
    without the team nothing is handed on at all."""
    held, handed = scenarios_why7()
    run_scenario(held, True, monkeypatch)
    run_scenario(handed, True, monkeypatch)
    run_scenario(handed, False, monkeypatch)


def test_the_next_sentence_of_a_workgroup(libs, monkeypatch):
    """A workgroup that handed a sentence on takes its next one with the same LDS, chunk tables and arena cursor: more sentences than the ordinary form's
    grid (they are claimed one by one, and a workgroup that gave up early claims the soonest), the handed ones of why 2, 6 and 8 in front."""
    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import DeviceContext

    monkeypatch.setenv("KGPU_POOL", "0")
    monkeypatch.setenv("KGPU_WINDOW_TEAM", "0")
    for make in (scenarios_why2, scenarios_why6, scenarios_why8):
        handed = [sc for sc in make() if sc.why][0]
        orc = handed.oracle()
        tok = Tokenizer(handed.dict)
        ctx = DeviceContext(tok)
        grid = ctx.plan()["window_workgroups"]
        k = 8 * len(handed.sentences)
        batch = handed.sentences * 8 + [ORDINARY[i % len(ORDINARY)] + "い" * (i % 37) + "漢x" * (i % 5) for i in range(grid + 64)]
        first, exp = run_batch(ctx, orc, batch)   # (a full grid's node chunks outgrow the arena's first size: this run may include a regrow, the next ones do not)
        again, _ = run_batch(ctx, orc, batch, exp)
        third, _ = run_batch(ctx, orc, batch, exp)
        print(f"{handed.name}: {k} + {grid + 64} sentences on a grid of {grid}: {first}, then {again}")
        assert again == third and again["deferred"] == [k, 0, 0, 0] == first["deferred"] and again["arena_regrows"] == 0, (first, again, third)
        assert again["window_handed"] == [k if i == handed.why else 0 for i in range(10)], again
        assert [v for i, v in enumerate(first["window_handed"]) if i not in (3, 5)] == [v for i, v in enumerate(again["window_handed"]) if i not in (3, 5)], first
        ctx.close()
        tok.close()


@pytest.mark.parametrize("window_kib", ["10", "0"], ids=["windowed", "general"])
def test_scratch_arena_too_small(libs, window_kib, monkeypatch):
    """KGPU_ARENA_INITIAL=1 MiB: the batch's chunks and slabs do not fit, the sentences that get none are flagged (why 3 / 5 with Control::arena_overflow in
    the windowed kernel, a refused slab in the general one), kgpu_ctx_sync doubles the arena and runs the batch again until it fits -- the caller sees the
    oracle's records and status 0.  The arena stays grown: a repeat on the same context regrows nothing."""
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.device import DeviceContext

    _, oracle = libs
    parts, plain, digits = arena_batches()
    d = Dict.from_parts(**parts)
    orc = oracle.OracleTokenizer.from_dict(d)
    monkeypatch.setenv("KGPU_POOL", "0")
    monkeypatch.setenv("KGPU_WINDOW", window_kib)
    monkeypatch.setenv("KGPU_WINDOW_TEAM", "0")
    monkeypatch.setenv("KGPU_ARENA_INITIAL", str(1 << 20))
    tok = Tokenizer(d)
    for batch in (plain, digits):
        ctx = DeviceContext(tok)   # (a context of its own: the arena is the context's, and starts at 1 MiB again)
        first, exp = run_batch(ctx, orc, batch)
        again, _ = run_batch(ctx, orc, batch, exp)
        print(f"KGPU_WINDOW={window_kib}: first {first}, again {again}")
        assert first["arena_regrows"] >= 1 and again["arena_regrows"] == 0
        assert first["deferred"] == [0] * 4 and again["deferred"] == [0] * 4 and first["tail_reruns"] == 0 and first["window_reruns"] == 0
        handed = first["window_handed"]
        if window_kib != "0":   # the runs that were given up counted the sentences they flagged for want of a chunk; nothing was handed on
            assert handed[3] + handed[5] >= 1 and sum(handed) == handed[3] + handed[5], first
        else:
            assert handed == [0] * 10
        assert again["window_handed"] == [0] * 10
        ctx.close()
    tok.close()


def test_where_a_handed_sentence_ends_up(libs):
    """Behind the pool kernel (the shipped chain): a sentence the windowed kernel hands on (why 6, the smallest) is served by the general kernel -- in a tail
    pass when the chain had been cut short (kgpu_routing.tail_reruns), in the chain itself once that is armed -- and the record consumers behind a host
    call render the final records."""
    import words_ref as W

    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.dictfile import MorphFeatureTable
    from kanpyo_amd.tokenizer import pack_sentences

    handed = [sc for sc in scenarios_why6() if sc.why][0]
    orc = handed.oracle()
    tok = Tokenizer(handed.dict)
    ctx = DeviceContext(tok)
    short = [ORDINARY[i % len(ORDINARY)] for i in range(40)]
    for _ in range(10):   # the windowed kernel starts armed; eight clean batches disarm it
        clean, _ = run_batch(ctx, orc, short)
        assert clean["tail_reruns"] == 0 and clean["window_handed"] == [0] * 10
    long_one = "辞書形態素テスト" * 40 + handed.sentences[0] + "x"   # too long for the pool kernel: it routes the sentence on
    mixed = short[:20] + [long_one] + short[20:]
    first, exp = run_batch(ctx, orc, mixed)
    assert first["tail_reruns"] == 1 and first["window_handed"] == [1 if i == 6 else 0 for i in range(10)] and first["deferred"][:2] == [1, 1], first
    again, _ = run_batch(ctx, orc, mixed, exp)   # armed now: the general kernel is in the chain
    assert again["tail_reruns"] == 0 and again["window_handed"] == first["window_handed"] and again["deferred"] == first["deferred"], again
    # the words renderer over a host call (a batch too large for the single-launch path): the lines are those of the oracle's records
    n_known, n_unk = len(handed.parts["sorted_keywords"]), len(handed.parts["unk_morphs"])
    known, unk = MorphFeatureTable.from_features([["名詞"]] * n_known), MorphFeatureTable.from_features([["未知"]] * n_unk)
    tok.set_features(known, unk)
    lines = mixed * 8
    utf8, offs = pack_sentences(lines)
    before = tok.routing(reset=True)
    text, toff, status = tok.words().render_packed(utf8, offs)
    e = orc.tokenize_batch(utf8, offs, 8)
    want, want_off = W.render(utf8, offs, e.tokens, e.offsets, known, unk, n_known, n_unk, W.Spec())
    assert not status.any() and np.array_equal(toff, want_off) and text.tobytes() == want
    assert tok.routing()["window_handed"][6] == 8, (before, tok.routing())
    ctx.close()
    tok.close()
