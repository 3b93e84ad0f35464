"""What the pool kernel's older tests know before a GPU is touched: the launch-chain knobs every kernel test clears, the plans and dictionaries of
tests/test_gpu_tile_groups.py (surface "あ" with k records: tile counts known by construction) and of tests/test_gpu_dead_positions.py (positions
nothing ends at), each with the reservation model's view of it (tests/pool_model.py through pool_cases.Dictionary).  tests/test_pool_model_cpu.py
checks these against the naive lattice without a device; tests/test_gpu_backtrace_quads.py reuses the dead-position dictionaries.  The windowed
kernel's cases are tests/window_cases.py, the pool front end's tests/pool_cases.py.  Nothing here needs a device or the GPU library at import."""
import functools

import numpy as np

import pool_cases as PC
import pool_model as M
from conftest import fixture_dict_parts

# the environment that shapes a launch chain: tests/kernel_run.py's set_env clears these before it sets a plan's
CHAIN_KNOBS = ("KGPU_POOL", "KGPU_WINDOW", "KGPU_WINDOW_TEAM", "KGPU_WINDOW_FIRST")

# ------------------------------------------------------------------------------------------------------------------------------------- tile groups
TILE_KS = list(range(1, 21)) + [31, 32, 33] + [63, 64, 65, 66]
TILE_NS = list(range(1, 13))
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
# needs a context that has seen a batch with an eighth of its sentences routed: every batch of these tests runs on a context of its own
# (kernel_run.run_fresh), so the model's 40:4:32 is what decides.
MODEL_PLANS = {"shipped": M.PLAN_SHIPPED, "pool80x8": (80 * 1024, 8, 20), "pool160x4": M.PLAN_160}


def tile_parts(k):
    kws = ["あ"] * k + ["い"]
    rng = np.random.default_rng(1000 + k)
    # few distinct costs: ties between predecessors in different chunks of a target group are common (first minimum in insertion order, lattice.rs:125,136)
    morphs = np.stack([rng.integers(0, 5, len(kws)), rng.integers(0, 5, len(kws)), rng.integers(-3, 4, len(kws)) * 100], axis=1)
    p = fixture_dict_parts()
    return dict(sorted_keywords=kws, morphs=morphs, conn_rows=5, conn_cols=5, conn_data=rng.integers(-2, 3, 25) * 50, char_class=p["char_class"],
                char_category=p["char_category"], invoke_list=p["invoke_list"], group_list=p["group_list"], unk_map={0: (1, 1), 1: (1, 2), 2: (2, 1)},
                unk_morphs=[[0, 0, 4000], [1, 1, 3500]])


def tile_sentences():
    """-> (plain, mixed).  plain, longest first: a pool workgroup's wavefronts take consecutive sentences, so the long ones share a pool and the later
    ones' pages lie high in it"""
    plain = ["あ" * n for n in reversed(TILE_NS)]
    mixed = ["あ" * 3 + "い" + "あ" * 2, "い" + "あ" * 4, "あい" * 3, "いい", "あ" * 5 + "い", "い", "あ" * 7 + "いい" + "あ"]
    return plain, mixed


@functools.lru_cache(maxsize=None)
def tile_model(k):
    """the reservation model's view of this dictionary (tests/pool_model.py over the lattice's shape; tests/test_pool_model_cpu.py checks that shape
    against the naive lattice)"""
    return PC.Dictionary(tile_parts(k))


def tile_predicted(k, plan, sentences):
    """-> (deferred[0], redone[0]) of one batch of these sentences on a fresh handle, by the model"""
    return M.counters([tile_model(k).verdict(s, MODEL_PLANS[plan])["verdict"] for s in sentences])


def tile_lds_need(k, chars):
    """Upper estimate of the pool kernel's LDS bytes for a sentence of `chars` characters, k records each (+ 3 for unknown words): text, the
    per-character arrays, 12 bytes a node, 8 a bucket entry, 8 a tile."""
    per = k + 3
    g = (per + 7) // 8
    return 3 * chars + 4 + 26 * (chars + 2) + 20 * (per * chars + 3) + 8 * (chars + 1) * g * g + 64


def tile_lds_floor(k, sentence):
    """Lower bound of the same for n x "あ" (0 for the mixed sentences): k nodes a position at 12 bytes, their bucket entries at 8, ceil(k / 8)^2
    tiles at 8 for every position but the first."""
    if set(sentence) != {"あ"}:
        return 0
    n, g = len(sentence), (k + 7) // 8
    return 20 * k * n + 8 * (n - 1) * g * g


# ---------------------------------------------------------------------------------------------------------------------------------- dead positions
BASES = ["あいう", "あいうあいう", "いあいう", "あいういう"]
DEAD_ORDINARY = ["", "あ", "い", "う", "いう", "うい", "ういあ", "いいい", "あいあ", "ううう", "あい", "いあ"]
DEAD_ENDS = ["テ", "テあ", "テ辞書", "テ辞書形態素", "テスト辞書", "ト辞書あ", "辞書テ", "形態素テ形態素", "テテ辞書辞書"]   # test_unreachable_eos_and_dead_ends
BEHIND_TE = ["テいう", "テあいう", "テいうあいう", "テあいういう", "いうテいう", "テう", "テい"]


def dead_parts(k, negative=False):
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


@functools.lru_cache(maxsize=None)
def dead_model(k, negative=False):
    """the reservation model's view of this dictionary (tests/pool_model.py; tests/test_pool_model_cpu.py checks its shapes against the naive lattice)"""
    return PC.Dictionary(dead_parts(k, negative))


def dead_need(pyref, pd, s):
    """Upper estimate of the pool kernel's LDS bytes for s, from the naive lattice: text, the per-character arrays, 12 bytes a node, 8 a bucket entry,
    8 a tile of a live position -- or, while the nodes are emitted, the match buffer (32 bytes a character) in the place of buckets and tiles."""
    tp, nodes, _, _ = M.shape(pyref, pd, s)
    C, N = len(s), len(nodes)
    tiles = sum(((t + 7) // 8) * ((p + 7) // 8) for t, p in tp)
    return 3 * C + 4 + 26 * (C + 2) + 12 * (N + 1) + max(8 * (N + 1) + 8 * tiles, 32 * C + 32) + 64


def dead_sentences(rng):
    """about 200: the four shapes 1 to 12 times repeated, mixed with ordinary ones"""
    out = [b * r for b in BASES for r in range(1, 13)]
    out += [b * r + o for b in BASES for r in (1, 2, 5) for o in ("い", "う", "あ")]
    while len(out) < 200:
        out.append("".join(rng.choice(DEAD_ORDINARY + BASES, size=int(rng.integers(1, 5)))))
    return [out[i] for i in rng.permutation(len(out))]
