"""The pool kernel's reservation model (tests/pool_model.py) and the cases chosen with it (tests/pool_cases.py), without a device: the model's own
arithmetic on pinned values, and for every case of tests/test_gpu_pool_limits.py what it claims -- which verdict each sentence gets, on which side
of which boundary it lies and by how many bytes -- by the model and the naive lattice (oracle/pyref.py) alone.  These assertions are what keeps a GPU
case from passing for the wrong reason: a sentence that stopped being REDONE, or is REDONE for another need than the case names, fails here first."""
import pytest

import kernel_cases as KC
import pool_cases as PC
import pool_model as M


def _pyref(parts):
    from kanpyo_amd import Dict
    from oracle import pyref

    d = Dict.from_parts(**parts)
    return pyref, pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)


# ------------------------------------------------------------------------------------------------------------------------------------------ the model
def test_page_sizes_and_limits():
    assert [M.page_bytes(p) for p in (M.PLAN_SHIPPED, M.PLAN_160, M.PLAN_SMALL)] == [624, 2544, 1016]
    assert M.page_bytes((80 * 1024, 8, 20)) == 1264 and M.page_bytes((20 * 1024, 2, 56)) == 304   # (kernel_cases.PLANS; the shipped chain's other shape)
    assert 32 * 624 == 19968 and 64 * 1016 == 65024 and 64 * 2544 == 162816
    # one wavefront: pages of 8 bytes' granularity, not 16 (1016 = 127 x 8 is no multiple of 16)
    assert M.page_bytes((64 * 1024, 4, 64)) == 1008


@pytest.mark.parametrize("page", [624, 2544, 1016, 304])
def test_pages_for_at_page_multiples(page):
    assert M.pages_for(0, page) == 0 and M.pages_for(1, page) == 1
    for k in (1, 2, 31, 32, 33, 63, 64, 65):
        assert [M.pages_for(k * page + d, page) for d in (-1, 0, 1)] == [k, k, k + 1]
    magic = (1 << 32) // page + 1   # launch_tokenize_pool's page_magic: the kernel's multiply-high is this division for every size a pool can meet
    for nbytes in list(range(0, 70 * page)) + [200000, 1 << 20]:
        assert ((nbytes + page - 1) * magic) >> 32 == M.pages_for(nbytes, page), nbytes


def test_tile_count_pinned_values():
    """the values tests/c_abi/tile_count.cpp and kgpu_tilepack.h's static_assert pin, and its count made the long way for T, P in 0..40"""
    pinned = {(0, 0): 0, (40, 0): 0, (0, 40): 0, (8, 8): 1, (9, 8): 2, (8, 9): 2, (40, 40): 25, (1, 0): 0, (0, 5): 0, (1, 1): 1, (17, 9): 6}
    assert {k: M.tile_count(*k) for k in pinned} == pinned
    for T in range(41):
        for P in range(41):
            assert M.tile_count(T, P) == len({(t // 8, p // 8) for t in range(T) for p in range(P)})


def test_steering_step_on_chain_policy_values():
    """tests/c_abi/chain_policy.cpp's est_after(late, est) checks with n = 1000 (there 7 stands for "no store": the estimate stays)"""
    E = 64 * 256
    assert M.steer(E, 251, 1000) == E + E // 4
    assert M.steer(E, 250, 1000) == E + E // 16
    assert M.steer(E, 32, 1000) == E + E // 16
    assert M.steer(E, 31, 1000) == E
    assert M.steer(E, 10, 1000) == E
    assert M.steer(E, 9, 1000) == E - E // 128
    assert M.steer(16 * 256, 0, 1000) == 16 * 256
    assert M.steer(16 * 256 + 4, 0, 1000) == 16 * 256
    assert M.steer(1024 * 256, 500, 1000) == 1024 * 256
    assert M.steer(1000 * 256, 500, 1000) == 1024 * 256


def test_need1_is_below_what_the_carve_takes():
    """kgpu_pool.hip:314: off + mbytes <= need1 by construction -- the per-character arrays and the match buffer of every sentence used fit need1"""
    for B, C in ((0, 0), (1, 1), (3, 1), (300, 100), (252, 252), (813, 271), (65000, 65000)):
        off = M.align_up(B + 4, 4) + 22 * (C + 2) + 2 * M.align_up(C + 2, 4)
        assert off + M.align_up(C * 32, 16) <= M.need1(B, C) <= off + C * 32 + 48


# --------------------------------------------------------------------------------------------------------------------------- the cases, by the model alone
def test_shapes_are_the_naive_lattice():
    """every sentence of every case: (T, P) per position from the key list (Shape) is what oracle/pyref.py's lattice has"""
    seen = {}
    h = PC.case_h()
    extra = [(h["d"], [h["held"], h["handed"]])]
    for d, sents in [(c.d, [s for b in c.batches for s in b.sentences]) for c in PC.all_cases()] + extra:
        key = id(d)
        if key not in seen:
            seen[key] = _pyref(d.parts)
        pyref, pd = seen[key]
        for s in dict.fromkeys(sents):
            assert d.look(s)[2] == M.shape(pyref, pd, s)[0], (len(s), s[:8])
            assert d.look(s)[0] == len(s.encode()) and d.look(s)[1] == len(s)


def test_ordinary_company_is_held():
    for c in PC.all_cases():
        for s in PC.SHORT:
            v = c.d.verdict(s, c.plan)
            assert v["verdict"] == M.HELD and v["npg"] <= 4, (c.name, s, v)


def test_case_a_routed_before_the_walk():
    c = PC.case_a()
    held, routed = (c.d.verdict(c.facts[k], c.plan) for k in ("held", "routed"))
    # est = 192 n + 768: n = 100 is the limit to the byte, n = 101 one page more
    assert held["est"] == 192 * 100 + 768 == 19968 == held["limit"] and held["npg"] == 32 and held["verdict"] == M.HELD
    assert routed["est"] == 192 * 101 + 768 and routed["npg"] == 33 and routed["verdict"] == M.ROUTED_BEFORE_WALK and routed["need_full"] is None
    assert held["need1"] < held["est"] and PC.margin(held) > 10000   # the estimate decides, not need1; the n = 100 lattice fits its 32 pages with room
    assert [(b.deferred0, b.redone0) for b in c.batches] == [(1, 0), (0, 0), (1, 0)]


@pytest.mark.parametrize("way", ["full", "emit", "short"])
def test_case_b_redo_from_both_sides(way):
    c = PC.case_b_pairs()[way]
    hs, rs = c.facts["held"], c.facts["redone"]
    held, redone = c.d.verdict(hs, c.plan), c.d.verdict(rs, c.plan)
    print(f"{way}: held {len(hs)} characters by {PC.margin(held)} bytes; redone {len(rs)} characters, short by {-PC.margin(redone)} bytes: {redone}")
    assert len(rs) == len(hs) + 1 and held["verdict"] == M.HELD and redone["verdict"] == M.REDONE
    assert 0 <= PC.margin(held) < held["page"] and 0 < -PC.margin(redone) < redone["page"]   # both within one page of the boundary
    assert redone["npg_redo"] == redone["npg"] + 1 <= 32                                     # ... and the redo asks for exactly one page more
    if way == "emit":
        assert redone["need_emit"] > redone["lds_bytes"] >= redone["need_full"]
    else:
        assert redone["need_full"] > redone["lds_bytes"] >= redone["need_emit"]
        # ... by so much that a redo sized by need_emit alone could not hold the sentence
        assert M.pages_for(redone["need_emit"], redone["page"]) * redone["page"] < redone["need_full"]
    if way == "full":
        assert not any(held["one_load"]) and not any(redone["one_load"]) and len(hs.encode()) >= 253
    if way == "short":
        assert all(held["one_load"]) and all(redone["one_load"]) and len(rs.encode()) <= 249
    assert [(b.deferred0, b.redone0) for b in c.batches] == [(0, 1), (0, 0), (0, 1)]


def test_case_b_mixed_batch_and_the_learning_runs():
    c = PC.case_b_mixed()
    (b,) = c.batches
    assert len(b.sentences) == 200 and b.deferred0 == 0 and set(b.labels) == {M.HELD, M.REDONE}
    runs = PC.learning_runs()
    print("learning runs:", [(est, r.redone0) for est, r in runs])
    assert runs[0][0] == M.EST_Q8_FRESH and runs[0][1].redone0 == b.redone0
    assert len({r.redone0 for _, r in runs}) == 3 and len({est for est, _ in runs}) == 3   # three different estimates, three different counts
    assert all(r.deferred0 == 0 and r.redone0 > 0 for _, r in runs)                        # nothing is routed under any of them
    assert [est for est, _ in runs][1:] == [M.steer(est, r.redone0, 200) for est, r in runs][:2]
    # EST_SLACK = 512 shifts the count (the mutant of DESIGN 6)
    assert M.counters([c.d.verdict(s, c.plan, est_slack=512)["verdict"] for s in b.sentences])[1] != b.redone0


def test_case_c_routed_after_the_walk():
    c = PC.case_c()
    routed, redone = (c.d.verdict(c.facts[k], c.plan) for k in ("routed", "redone"))
    assert len(c.facts["routed"]) == len(c.facts["redone"]) + 1
    assert routed["verdict"] == M.ROUTED_AFTER_WALK and routed["npg"] <= 32 < routed["npg_redo"] == 33
    assert redone["verdict"] == M.REDONE and redone["npg"] < redone["npg_redo"] == 32
    assert 0 < max(routed["need_emit"], routed["need_full"]) - routed["limit"] < routed["page"]   # beyond the limit by less than a page
    assert 0 <= redone["limit"] - max(redone["need_emit"], redone["need_full"]) < redone["page"]  # ... and within it by less than a page
    assert [(b.deferred0, b.redone0) for b in c.batches] == [(1, 2), (1, 1), (0, 1)]


def test_case_d_every_wavefront_redoes():
    c = PC.case_d()
    v = c.d.verdict(c.facts["sentence"], c.plan)
    assert v["verdict"] == M.REDONE and 30 <= v["npg_redo"] <= 32 and v["npg"] < v["npg_redo"]
    assert 2 * v["npg"] <= 64 < 3 * v["npg"] and 2 * v["npg_redo"] <= 64 < 3 * v["npg_redo"]   # two reservations fit a pool, a third does not
    (b,) = c.batches
    assert len(b.sentences) == 64 and (b.deferred0, b.redone0) == (0, 64)


def test_case_e_maxm():
    c = PC.case_e()
    held, handed = c.facts["held"], c.facts["handed"]
    assert [len(p) for p in c.d.look(held)[3]] == [8, 7, 6, 5, 4, 3, 2, 1] and [len(p) for p in c.d.look(handed)[3]][:2] == [9, 8]
    assert c.d.verdict(held, c.plan)["verdict"] == M.HELD and c.d.verdict(handed, c.plan)["verdict"] == M.ROUTED_MATCHES
    assert c.d.verdict(handed, c.plan)["npg"] <= 32   # (the reservation is not what hands it on)
    assert [(b.deferred0, b.redone0) for b in c.batches] == [(0, 0), (1, 0), (2, 0)]


def test_cases_f_the_rider():
    for c in PC.cases_f():
        deepest, unk = c.facts["deepest"], c.facts["unk"]
        pyref, pd = _pyref(c.parts)
        first = "あ" * deepest
        tp = c.d.look(first)[2]
        assert len(c.d.look(first)[3][0]) == deepest and tp[0][0] == deepest + unk, (c.name, tp)   # `deepest` prefixes and the unknown records start at 0
        assert unk == pd.unk[2][1] and pd.invoke[2]
        (b,) = c.batches
        assert b.deferred0 == 0 and all(M.parks_every_match(c.d.look(s)[3]) for s in b.sentences)
        # the unknown records matter: the best path of one of the sentences takes one at a position that has dictionary prefixes too
        taken = [t for s in c.facts["sentences"] for t in pyref.tokenize(pd, s) if t[1] == 2 and s[t[3]] == "あ"]
        assert taken, c.name


def test_cases_g_the_8_bit_length():
    held, handed = PC.cases_g()
    for s in held.facts["sentences"]:
        assert max(n for p in held.d.look(s)[3] for n in p) == 255 and held.d.verdict(s, held.plan)["verdict"] == M.HELD
    (s,) = handed.facts["sentences"]
    assert handed.d.look(s)[3][0] == [256] and handed.d.verdict(s, handed.plan)["verdict"] == M.ROUTED_MATCHES
    assert [(b.deferred0, b.redone0) for b in held.batches] == [(0, 0)] and [(b.deferred0, b.redone0) for b in handed.batches] == [(1, 0), (0, 0)]
    assert handed.batches[0].expect()["window_handed"][2] == 1 and handed.batches[0].expect()["deferred"] == [1, 1, 0, 0]
    assert all(len(s.encode()) < 1024 for s in held.facts["sentences"])   # (and KGPU_WINDOW_FIRST=0 besides: the batch starts with the pool kernel)


def test_case_h_the_small_call():
    h = PC.case_h()
    held, handed = h["d"].verdict(h["held"], h["plan"]), h["d"].verdict(h["handed"], h["plan"])
    print(f"small call: held {len(h['held'])} characters, {held['need_full']} of 65024 bytes; handed {handed['need_full']}")
    assert held["page"] == 1016 and held["npg"] == 64 and held["lds_bytes"] == 65024
    assert held["verdict"] == M.HELD and 0 <= PC.margin(held) < 256
    assert handed["verdict"] == M.ROUTED_AFTER_WALK and 0 < -PC.margin(handed) < 256 and handed["need1"] <= 65024   # not need1: the exact need hands it on
    assert len(h["handed"].encode()) < 16 * 1024   # a small call still
    # the general path behind a fallback: the shipped plan's pool kernel routes that sentence before the walk
    assert h["d"].verdict(h["handed"], M.PLAN_SHIPPED)["verdict"] == M.ROUTED_BEFORE_WALK


# --------------------------------------------------------------------------------- the two older modules whose counters are the model's (tests/kernel_cases.py)
def test_tile_groups_batches_by_the_model():
    """what test_gpu_tile_groups.py asks of the device, by the model alone: none of the sentences meant for the pool kernel is routed, and of the longer
    ones at least those whose nodes, bucket entries and tiles alone exceed the limit are; the shapes are the naive lattice's."""
    plain, mixed = KC.tile_sentences()
    redone = 0
    for k in KC.TILE_KS:
        if k in (1, 8, 9, 33, 66):
            pyref, pd = _pyref(KC.tile_parts(k))
            for s in plain[:2] + mixed:
                assert KC.tile_model(k).look(s)[2] == M.shape(pyref, pd, s)[0], (k, s)
        for plan, mp in KC.MODEL_PLANS.items():
            assert M.page_bytes(mp) * mp[2] == KC.PLANS[plan][1]
            limit = KC.PLANS[plan][1]
            inside = [s for s in plain + mixed if KC.tile_lds_need(k, len(s)) * 6 <= limit * 5]
            beyond = [s for s in plain + mixed if s not in inside]
            want = KC.tile_predicted(k, plan, inside)
            assert want[0] == 0, (k, plan, want)
            redone += want[1]
            if beyond:
                must = sum(1 for s in beyond if KC.tile_lds_floor(k, s) > limit)
                assert must <= KC.tile_predicted(k, plan, beyond)[0] <= len(beyond), (k, plan)
    assert redone > 0   # the equality is about something: some of these batches do redo sentences


def test_dead_positions_batches_by_the_model():
    """test_gpu_dead_positions.py's dictionaries: the model's shapes are the naive lattice's (dead positions, unreachable nodes and all)"""
    import numpy as np

    for k, negative in ((1, False), (9, False), (17, True), (8, True)):
        pyref, pd = _pyref(KC.dead_parts(k, negative))
        sents = KC.BASES + KC.dead_sentences(np.random.default_rng(k))[:40] + (KC.DEAD_ENDS + KC.BEHIND_TE if negative else [])
        for s in sents:
            assert KC.dead_model(k, negative).look(s)[2] == M.shape(pyref, pd, s)[0], (k, negative, s)
