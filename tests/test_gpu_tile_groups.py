"""Stage B's tile groups (kanpyo_amd/csrc/kgpu_device.h: tiles_run -- descriptors in windows of 64, gathered a group ahead of the sweep), bit-exact
against the oracle on lattices whose tile counts are known by construction.

The dictionary's surface "あ" has k records (and "い" one), so in a sentence of n x "あ" every inner position has T = P = k: ceil(k / 8)^2 tiles a
position, n x ceil(k / 8)^2 (+ the first position's ceil(k / 8) and EOS's ceil(k / 8)) a sentence -- with k in 1..20, 31..33, 63..66 and n in 1..12 the
counts cross every multiple of the group size (4; 8 before) and of the 64-descriptor window, and a target group has 1..9 chunks and starts at every
phase of a group.  The sentences with "い" put a many-chunk target group (T = 1, P = k) directly in front of single-chunk ones (EOS; or T = k, P = 1
behind it): what is gathered ahead for the next group must not read a node the sweep of this group has just written (the padding node of round 6).

Which kernel served a batch is asserted from the routing counters (DeviceContext.profile: `deferred`), not assumed: on the pool plans only sentences
whose LDS need is safely below the plan's routing limit are in the asserted batch (kernel_cases.tile_lds_need, with a fifth of margin, against
max pages x page bytes of the plan); the longer ones run in a batch of their own with the windowed kernel behind the pools: those that cannot fit
the pool must have left it, and none may reach the general kernel.  How many of a batch the pool kernel redoes and how many it hands on is asserted as
the exact number tests/pool_model.py predicts (a fresh handle and one batch; tests/test_gpu_pool_limits.py aims at the limits themselves).
test_pool_addresses_above_64k pins the upper half-word range of the address pack:
one sentence whose node array alone is longer than 64 KB, served by a 160 KB pool."""
import pytest

from kernel_cases import PLANS, TILE_KS, tile_lds_floor, tile_lds_need, tile_parts, tile_predicted, tile_sentences
from kernel_run import libs, run_fresh, set_env  # noqa: F401  (libs: the fixture)

pytestmark = pytest.mark.gpu


def _dict(k):
    from kanpyo_amd import Dict

    return Dict.from_parts(**tile_parts(k))


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("k", TILE_KS)
def test_tile_groups(libs, k, plan, monkeypatch):
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    env, limit = PLANS[plan]
    set_env(monkeypatch, env)
    d = _dict(k)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    plain, mixed = tile_sentences()
    sents = plain + mixed
    try:
        if limit is None:
            prof = run_fresh(tok, orc, sents)
            print(f"k={k} {plan}: deferred {prof['deferred']} long_launches {prof['long_launches']}")
            assert prof["long_launches"] == 1, prof
            # the windowed kernel served every sentence: nothing went on to the general kernel (list 0; behind the team form list 1 -- its list 0 is
            # what the team form handed to the ordinary one)
            assert prof["deferred"][1 if plan == "window_team" else 0] == 0, prof
        else:
            inside = [s for s in sents if tile_lds_need(k, len(s)) * 6 <= limit * 5]
            beyond = [s for s in sents if s not in inside]
            assert len(inside) >= 8 and "あ" in inside, (k, plan)
            prof = run_fresh(tok, orc, inside)
            print(f"k={k} {plan}: {len(inside)} sentences meant for the pool kernel: deferred {prof['deferred']} redone {prof['redone']}; {len(beyond)} beyond")
            assert prof["deferred"][0] == 0, prof   # the pool kernel served every one of them: none left it for the windowed kernel
            # ... and redid (reservation too small) exactly those the model says: a fresh handle and one batch
            assert tile_predicted(k, plan, inside)[0] == 0
            assert sum(prof["deferred"]) == 0 and prof["redone"][0] == tile_predicted(k, plan, inside)[1], (prof, tile_predicted(k, plan, inside))
            if beyond:
                # The longer ones: the pool kernel first, the windowed kernel (24 KB, as in the window plans: it holds four positions of 66 records)
                # behind it.  Asserted: a sentence whose nodes, bucket entries and tiles ALONE exceed the pool's routing limit left the pool kernel,
                # no more than the batch did, and none reached the general kernel -- every one was swept by one of the two LDS kernels' tiles_run.
                monkeypatch.setenv("KGPU_WINDOW", "24")
                tok2 = Tokenizer(d)
                try:
                    prof = run_fresh(tok2, orc, beyond)
                finally:
                    tok2.close()
                must = sum(1 for s in beyond if tile_lds_floor(k, s) > limit)
                print(f"k={k} {plan}: beyond the limit: deferred {prof['deferred']} redone {prof['redone']}; {must} of {len(beyond)} cannot fit the pool")
                want = tile_predicted(k, plan, beyond)   # (tok2 is a fresh handle as well)
                assert must <= want[0] <= len(beyond) and prof["deferred"][0] == want[0], (must, want, prof)
                assert prof["deferred"][1] == 0 and prof["deferred"][2] == 0 and prof["deferred"][3] == 0, prof
                assert prof["redone"][0] == want[1], (want, prof)
    finally:
        tok.close()


def test_pool_addresses_above_64k(libs, monkeypatch):
    """LDS addresses above 64 KB by construction, not by luck of the page allocator: k = 18 records on "あ", 310 characters -> at least 18 x 310 nodes
    of 12 bytes = 66 960 bytes of node arrays in ONE contiguous reservation, so the last nodes and EVERY bucket entry (the buckets follow the nodes) lie
    above byte 65 536 of the workgroup's LDS wherever the reservation starts; the upper estimate of the whole lattice (153 KB) fits the 160 KB pool's
    64 pages (162 816 bytes).  The routing counters must show that the pool kernel served it (nothing deferred): then 16-bit byte addresses would
    have been wrong, and the 8-byte units are what made the records right."""
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    k, chars = 18, 310
    assert 12 * k * chars > 65536 and tile_lds_need(k, chars) <= 64 * 2544
    set_env(monkeypatch, {"KGPU_POOL": "160:4", "KGPU_WINDOW_FIRST": "0"})   # (the batch's average length must not send it to the windowed kernel first)
    d = _dict(k)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    try:
        prof = run_fresh(tok, orc, ["あ" * chars, "あ" * (chars - 7) + "い" + "あ" * 6, "あ" * 5])
        print(f"k={k} 160:4, {chars} characters: deferred {prof['deferred']} redone {prof['redone']}")
        assert sum(prof["deferred"]) == 0, prof
    finally:
        tok.close()
