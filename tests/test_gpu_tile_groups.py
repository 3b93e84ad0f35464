"""Stage B's tile groups (kanpyo_amd/csrc/kgpu_device.h: tiles_run -- descriptors in windows of 64, gathered a group ahead of the sweep), bit-exact
against the oracle on lattices whose tile counts are known by construction.

The dictionary's surface "あ" has k records (and "い" one), so in a sentence of n x "あ" every inner position has T = P = k: ceil(k / 8)^2 tiles a
position, n x ceil(k / 8)^2 (+ the first position's ceil(k / 8) and EOS's ceil(k / 8)) a sentence -- with k in 1..20, 31..33, 63..66 and n in 1..12 the
counts cross every multiple of the group size (4; 8 before) and of the 64-descriptor window, and a target group has 1..9 chunks and starts at every
phase of a group.  The sentences with "い" put a many-chunk target group (T = 1, P = k) directly in front of single-chunk ones (EOS; or T = k, P = 1
behind it): what is gathered ahead for the next group must not read a node the sweep of this group has just written (the padding node of round 6).

Which kernel served a batch is asserted from the routing counters (DeviceContext.profile: `deferred`), not assumed: on the pool plans only sentences
whose LDS need is safely below the plan's routing limit are in the asserted batch (the estimate below, with a fifth of margin, against
max pages x page bytes of the plan); the longer ones run in a batch of their own with the windowed kernel behind the pools: those that cannot fit
the pool must have left it, and none may reach the general kernel.  How many of a batch the pool kernel redoes and how many it hands on is asserted as
the exact number tests/pool_model.py predicts (a fresh handle and one batch; tests/test_gpu_pool_limits.py aims at the limits themselves).
test_pool_addresses_above_64k pins the upper half-word range of the address pack:
one sentence whose node array alone is longer than 64 KB, served by a 160 KB pool."""
import functools

import numpy as np
import pytest

import pool_cases as PC
import pool_model as M
from conftest import fixture_dict_parts

pytestmark = pytest.mark.gpu

KS = list(range(1, 21)) + [31, 32, 33] + [63, 64, 65, 66]
NS = list(range(1, 13))
# plan -> (environment, bytes a sentence may take in the first kernel of the chain or None: no pool kernel)
#   page = ((KiB * 1024 - 16) / 64) rounded down to 16 bytes, limit = max pages x page (kgpu_pool.hip: launch_tokenize_pool; kgpu_chain.cpp: make_plan)
PLANS = {
    "shipped": ({}, 32 * 624),
    "pool80x8": ({"KGPU_POOL": "80:8:20"}, 20 * 1264),
    "pool160x4": ({"KGPU_POOL": "160:4"}, 64 * 2544),
    "window": ({"KGPU_POOL": "0", "KGPU_WINDOW": "24", "KGPU_WINDOW_TEAM": "0"}, None),
    "window_team": ({"KGPU_POOL": "0", "KGPU_WINDOW": "24", "KGPU_WINDOW_TEAM": "2"}, None),
}
# the pool plans as tests/pool_model.py takes them: (pool bytes, wavefronts, max pages).  "shipped" leaves KGPU_POOL unset, so the chain may pick the
# pool's shape per batch (kgpu_chain.cpp: build_chain) -- three wavefronts instead of four share the same pages of 624 bytes, and the 20 KB shape
# needs a context that has seen a batch with an eighth of its sentences routed: every batch here runs on a context of its own (_run), so the
# model's 40:4:32 is what decides.
MODEL_PLANS = {"shipped": M.PLAN_SHIPPED, "pool80x8": (80 * 1024, 8, 20), "pool160x4": M.PLAN_160}


@pytest.fixture(scope="module")
def libs():
    from kanpyo_amd import _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    from oracle import oracle

    oracle.build()
    return _lib, oracle


def _parts(k):
    kws = ["あ"] * k + ["い"]
    rng = np.random.default_rng(1000 + k)
    # few distinct costs: ties between predecessors in different chunks of a target group are common (first minimum in insertion order, lattice.rs:125,136)
    morphs = np.stack([rng.integers(0, 5, len(kws)), rng.integers(0, 5, len(kws)), rng.integers(-3, 4, len(kws)) * 100], axis=1)
    p = fixture_dict_parts()
    return dict(sorted_keywords=kws, morphs=morphs, conn_rows=5, conn_cols=5, conn_data=rng.integers(-2, 3, 25) * 50, char_class=p["char_class"],
                char_category=p["char_category"], invoke_list=p["invoke_list"], group_list=p["group_list"], unk_map={0: (1, 1), 1: (1, 2), 2: (2, 1)},
                unk_morphs=[[0, 0, 4000], [1, 1, 3500]])


def _dict(k):
    from kanpyo_amd import Dict

    return Dict.from_parts(**_parts(k))


@functools.lru_cache(maxsize=None)
def _model(k):
    """the reservation model's view of this dictionary (tests/pool_model.py over the lattice's shape; tests/test_pool_model_cpu.py checks that shape
    against the naive lattice)"""
    return PC.Dictionary(_parts(k))


def _predicted(k, plan, sentences):
    """-> (deferred[0], redone[0]) of one batch of these sentences on a fresh handle, by the model"""
    return M.counters([_model(k).verdict(s, MODEL_PLANS[plan])["verdict"] for s in sentences])


def _lds_need(k, chars):
    """Upper estimate of the pool kernel's LDS bytes for a sentence of `chars` characters, k records each (+ 3 for unknown words): text, the
    per-character arrays, 12 bytes a node, 8 a bucket entry, 8 a tile."""
    per = k + 3
    g = (per + 7) // 8
    return 3 * chars + 4 + 26 * (chars + 2) + 20 * (per * chars + 3) + 8 * (chars + 1) * g * g + 64


def _lds_floor(k, sentence):
    """Lower bound of the same for n x "あ" (0 for the mixed sentences): k nodes a position at 12 bytes, their bucket entries at 8, ceil(k / 8)^2
    tiles at 8 for every position but the first."""
    if set(sentence) != {"あ"}:
        return 0
    n, g = len(sentence), (k + 7) // 8
    return 20 * k * n + 8 * (n - 1) * g * g


def _run(tok, orc, sentences):
    import torch

    from kanpyo_amd.device import PROFILE_OFF, DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sentences)
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(utf8.copy()).to(dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    n, cap = len(sentences), int(offs[-1]) + len(sentences)
    d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx = DeviceContext(tok)
    ctx.set_profiling(PROFILE_OFF)
    ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
    nt = ctx.sync()
    exp = orc.tokenize_batch(utf8, offs, 2)
    assert not d_st.cpu().numpy().any()
    assert np.array_equal(d_toff.cpu().numpy().astype(np.uint64), exp.offsets), "per-sentence token counts differ"
    got = d_tok[:nt].cpu().numpy().reshape(-1)
    want = exp.tokens.view(np.int32).reshape(-1)
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0]) // 6
        s = int(np.searchsorted(exp.offsets, bad, side="right") - 1)
        raise AssertionError(f"token {bad} (sentence {s}: {sentences[s]!r}) differs: gpu {got[6 * bad:6 * bad + 6]} oracle {want[6 * bad:6 * bad + 6]}")
    prof = ctx.profile()
    ctx.close()
    return prof


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("k", KS)
def test_tile_groups(libs, k, plan, monkeypatch):
    from kanpyo_amd import Tokenizer

    _, oracle = libs
    env, limit = PLANS[plan]
    for name in ("KGPU_POOL", "KGPU_WINDOW", "KGPU_WINDOW_TEAM", "KGPU_WINDOW_FIRST"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    d = _dict(k)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    # longest first: a pool workgroup's wavefronts take consecutive sentences, so the long ones share a pool and the later ones' pages lie high in it
    plain = ["あ" * n for n in reversed(NS)]
    mixed = ["あ" * 3 + "い" + "あ" * 2, "い" + "あ" * 4, "あい" * 3, "いい", "あ" * 5 + "い", "い", "あ" * 7 + "いい" + "あ"]
    sents = plain + mixed
    try:
        if limit is None:
            prof = _run(tok, orc, sents)
            print(f"k={k} {plan}: deferred {prof['deferred']} long_launches {prof['long_launches']}")
            assert prof["long_launches"] == 1, prof
            # the windowed kernel served every sentence: nothing went on to the general kernel (list 0; behind the team form list 1 -- its list 0 is
            # what the team form handed to the ordinary one)
            assert prof["deferred"][1 if plan == "window_team" else 0] == 0, prof
        else:
            inside = [s for s in sents if _lds_need(k, len(s)) * 6 <= limit * 5]
            beyond = [s for s in sents if s not in inside]
            assert len(inside) >= 8 and "あ" in inside, (k, plan)
            prof = _run(tok, orc, inside)
            print(f"k={k} {plan}: {len(inside)} sentences meant for the pool kernel: deferred {prof['deferred']} redone {prof['redone']}; {len(beyond)} beyond")
            assert prof["deferred"][0] == 0, prof   # the pool kernel served every one of them: none left it for the windowed kernel
            # ... and redid (reservation too small) exactly those the model says: a fresh handle and one batch
            assert _predicted(k, plan, inside)[0] == 0
            assert sum(prof["deferred"]) == 0 and prof["redone"][0] == _predicted(k, plan, inside)[1], (prof, _predicted(k, plan, inside))
            if beyond:
                # The longer ones: the pool kernel first, the windowed kernel (24 KB, as in the window plans: it holds four positions of 66 records)
                # behind it.  Asserted: a sentence whose nodes, bucket entries and tiles ALONE exceed the pool's routing limit left the pool kernel,
                # no more than the batch did, and none reached the general kernel -- every one was swept by one of the two LDS kernels' tiles_run.
                monkeypatch.setenv("KGPU_WINDOW", "24")
                tok2 = Tokenizer(d)
                try:
                    prof = _run(tok2, orc, beyond)
                finally:
                    tok2.close()
                must = sum(1 for s in beyond if _lds_floor(k, s) > limit)
                print(f"k={k} {plan}: beyond the limit: deferred {prof['deferred']} redone {prof['redone']}; {must} of {len(beyond)} cannot fit the pool")
                want = _predicted(k, plan, beyond)   # (tok2 is a fresh handle as well)
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
    assert 12 * k * chars > 65536 and _lds_need(k, chars) <= 64 * 2544
    for name in ("KGPU_WINDOW", "KGPU_WINDOW_TEAM"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("KGPU_POOL", "160:4")
    monkeypatch.setenv("KGPU_WINDOW_FIRST", "0")   # (the batch's average length must not send it to the windowed kernel first)
    d = _dict(k)
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    try:
        prof = _run(tok, orc, ["あ" * chars, "あ" * (chars - 7) + "い" + "あ" * 6, "あ" * 5])
        print(f"k={k} 160:4, {chars} characters: deferred {prof['deferred']} redone {prof['redone']}")
        assert sum(prof["deferred"]) == 0, prof
    finally:
        tok.close()
