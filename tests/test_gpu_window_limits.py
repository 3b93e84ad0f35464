"""The windowed kernel's hand-on limits (kanpyo_amd/csrc/kgpu_window.hip), each reached on purpose and told apart by kgpu_routing.window_handed.

The kernel holds a sentence of any length in a bounded LDS; what it cannot hold it pushes onto the next launch's work list and counts under the
limit it ran into (`why`, codes 1-8, the table at kgpu_routing in include/kanpyo_gpu.h).  Every exit is a `break` out of a loop that holds LDS
state, prefetched registers and -- in the two-wavefront (TEAM) form -- two tokens another wavefront polls, so every case here is a PAIR on tiny
dictionaries (Dict.from_parts): a HELD sentence just inside the limit (nothing deferred, every counter 0) and a HANDED one just outside it (exactly
the intended counter, every other one 0), between ordinary sentences, bit-exact against the oracle (records, offsets, status: no tolerance), run
twice with identical routing.  KGPU_POOL=0: every sentence enters the windowed kernel, so deferred[0] is what it handed on; with
KGPU_WINDOW_TEAM=2 the team hands to list 0 and the ordinary form behind it to list 1 (a sentence neither holds is counted twice).

Which side of a limit a sentence is on is decided BEFORE the GPU is touched, from a plain-Python model of the lattice's shape (`shape`: the nodes
per start position from the key list, the category table and the unknown-word rules of src/lattice.rs:42-99) whose node total must equal the
oracle's (counters["N"]) for every sentence: the scenarios() functions, which tests/test_window_limits_cpu.py runs without a device.  A change to a
dictionary builder then cannot turn a case into a no-op.

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

from conftest import fixture_dict_parts

pytestmark = pytest.mark.gpu

# kgpu_window.hip's constants, as its header documents them
WIN, WMAXM, XMAX, NEARLEN = 32, 8, 48, 32
NODE_LIMIT = 32 << 13            # NCHUNKS << NCH_LOG: gw + N (BOS included) must stay below
FIFO_LIMIT = (16 - 1) << 12      # (FCHUNKS - 1) << FCH_LOG far entries waiting
REBASE = 0x8000                  # node indices inside a window are 16-bit offsets from (first node of the window) - 0x8000
CCAP = 384                       # TEAM form: entries of a carry bank
MAX_UNKNOWN_LEN = 1024
WINDOW_LDS_DEFAULT = 10 * 1024   # KGPU_WINDOW's default (kgpu_chain.cpp); the GPU tests check the plan against it
ORDINARY = ["テスト", "", "漢字かな", "xyz テスト", "いうえお", "辞書x形態素"]   # (no あ, no digit: the cases' dictionaries make those heavy)


# ---------------------------------------------------------------------------------------------------------------- dictionaries and the shape model
def make_parts(keys, invoke=(0, 1, 0), group=(0, 1, 0), unk=(1, 1, 1), seed=1, digits_cat=None):
    """Dict.from_parts arguments over the fixture's three categories (0 DEFAULT, 1 KANJI, 2 HIRAGANA).  keys: [(surface, records)];
    invoke / group: per category; unk: unknown records per category; digits_cat: the category '0'..'9' get."""
    rng = np.random.default_rng(seed)
    R = 4
    kws = sorted([k for k, dup in keys for _ in range(dup)], key=lambda s: s.encode())
    morphs = np.stack([rng.integers(0, R, len(kws)), rng.integers(0, R, len(kws)), rng.integers(-500, 5000, len(kws))], axis=1)
    p = fixture_dict_parts()
    cat = p["char_category"].copy()
    if digits_cat is not None:
        cat[0x30:0x3A] = digits_cat
    unk_map, unk_morphs = {}, []
    for c, k in enumerate(unk):
        if k:
            unk_map[c] = (len(unk_morphs) + 1, k)
            unk_morphs += [[int(rng.integers(0, R)), int(rng.integers(0, R)), int(rng.integers(3000, 6000))] for _ in range(k)]
    return dict(sorted_keywords=kws, morphs=morphs, conn_rows=R, conn_cols=R, conn_data=rng.integers(-900, 900, R * R), char_class=p["char_class"],
                char_category=cat, invoke_list=np.array(invoke, dtype=np.uint8), group_list=np.array(group, dtype=np.uint8), unk_map=unk_map,
                unk_morphs=unk_morphs)


class Shape:
    """The lattice's shape from the key list alone: per start position the dictionary prefixes [(chars, records)] in ascending length and the
    unknown words (span, records); src/lattice.rs:42-99.  Node order is insertion order: position by position, prefixes, then unknown words."""

    def __init__(self, parts, text):
        keys = {}
        for k in parts["sorted_keywords"]:
            keys[k] = keys.get(k, 0) + 1
        lens = sorted({len(k) for k in keys})
        cat = [int(parts["char_category"][ord(c)]) for c in text]
        C = len(text)
        run = [0] * (C + 1)
        for i in range(C - 1, -1, -1):
            run[i] = min(MAX_UNKNOWN_LEN, 1 + (run[i + 1] if i + 1 < C and cat[i + 1] == cat[i] else 0))
        self.C, self.prefixes, self.unknown = C, [], []
        for i in range(C):
            pre = [(n, keys[text[i : i + n]]) for n in lens if i + n <= C and text[i : i + n] in keys]
            u = (0, 0)
            if (not pre or parts["invoke_list"][cat[i]]) and cat[i] in parts["unk_map"]:
                u = (run[i] if parts["group_list"][cat[i]] else 1, parts["unk_map"][cat[i]][1])
            self.prefixes.append(pre)
            self.unknown.append(u)
        # every node but BOS / EOS: (start, end, index) with BOS = node 0
        self.per_pos = [sum(r for _, r in self.prefixes[i]) + self.unknown[i][1] for i in range(C)]
        self.first = np.concatenate([[1], 1 + np.cumsum(self.per_pos)]).astype(np.int64)   # first[i]: index of position i's first node; first[C]: EOS
        self.nodes_with_bos = int(self.first[C]) + 1
        self._near = None

    def entries(self):
        """(start, end, node index) of every node in insertion order."""
        for i in range(self.C):
            g = int(self.first[i])
            for n, r in self.prefixes[i]:
                for _ in range(r):
                    yield i, i + n, g
                    g += 1
            for _ in range(self.unknown[i][1]):
                yield i, i + self.unknown[i][0], g
                g += 1

    def far(self):
        return [(s, e, g) for s, e, g in self.entries() if e - s > NEARLEN]

    def parked(self, w0, nw=WIN):
        """Matches a window [w0, w0 + nw) parks in its shared overflow area: the ninth prefix and beyond of every position."""
        return sum(max(0, len(self.prefixes[i]) - WMAXM) for i in range(w0, min(self.C, w0 + nw)))

    def far_ends_never_decrease(self):
        ends = [e for _, e, _ in self.far()]
        return all(a <= b for a, b in zip(ends, ends[1:]))

    def fifo_waiting(self):
        """-> (lo[p], hi[p]) per position p: far entries alive at p (start <= p <= end) -- in the FIFO when the window that holds p is flushed,
        however the windows are cut -- and those with start < p + WIN and end >= p: an upper bound for a window that starts at p."""
        lo, hi = np.zeros(self.C + 2, dtype=np.int64), np.zeros(self.C + 2, dtype=np.int64)
        for s, e, _ in self.far():
            lo[s] += 1; lo[min(e, self.C) + 1] -= 1
            hi[max(0, s - WIN + 1)] += 1; hi[min(e, self.C) + 1] -= 1
        return np.cumsum(lo)[: self.C + 1], np.cumsum(hi)[: self.C + 1]

    def seed_gaps(self):
        """Per far entry that ends inside the sentence: (least, most) distance between its node index and the first node of the window its end falls
        in -- the window starts at most WIN - 1 positions before that end."""
        out = []
        for s, e, g in self.far():
            if e <= self.C:
                out.append((int(self.first[max(0, e - WIN + 1)]) - g, int(self.first[e]) - g))
        return out

    def carried(self, b):
        """Bucket entries a window that ends in front of position b carries on: near nodes with start < b <= end."""
        if self._near is None:
            self._near = [(s, e) for s, e, _ in self.entries() if e - s <= NEARLEN]
        return sum(1 for s, e in self._near if s < b <= e)


class Scenario:
    """One dictionary, its sentences with the limit they are expected to run into (0: held), and the environment beyond KGPU_POOL=0."""

    def __init__(self, name, parts, sentences, why, env=None, lds=WINDOW_LDS_DEFAULT, team_why=None):
        self.name, self.parts, self.sentences, self.why, self.env, self.lds = name, parts, sentences, why, dict(env or {}), lds
        self.team_why = why if team_why is None else team_why   # what the team form runs into (the ordinary form behind it then meets `why`, or holds the sentence)

    def oracle(self):
        from kanpyo_amd import Dict
        from oracle import oracle

        oracle.build()
        self.dict = Dict.from_parts(**self.parts)
        self.orc = oracle.OracleTokenizer.from_dict(self.dict)
        return self.orc

    def shapes(self):
        """The model of every special sentence, checked against the oracle's node count (counters N: every node but BOS)."""
        orc = self.oracle()
        out = []
        for s in self.sentences:
            sh = Shape(self.parts, s)
            _, ctr = orc.tokenize(s)
            assert ctr["N"] + 1 == sh.nodes_with_bos, (self.name, len(s), ctr, sh.nodes_with_bos)
            out.append(sh)
        return out


def scenarios_why2():
    """why 2: the window's shared overflow area.  Keys あ^1..あ^10: a position inside a run has min(10, what is left) prefixes, the ninth and tenth are
    parked; windows start at multiples of WIN while none is shortened."""
    parts = make_parts([("あ" * n, 1) for n in range(1, 11)], invoke=(0, 1, 0), group=(0, 1, 0), seed=2)
    held = Scenario("why2 held", parts, ["あ" * 32, "x" * 8 + "あ" * 33], 0)
    handed = Scenario("why2 handed", parts, ["あ" * 33, "x" * 7 + "あ" * 33], 2)
    assert [sh.parked(0) for sh in held.shapes()] == [XMAX - 1, XMAX]
    assert all(max(sh.parked(w) for w in range(0, sh.C, WIN)) <= XMAX for sh in held.shapes())
    assert [sh.parked(0) for sh in handed.shapes()] == [XMAX + 1, XMAX + 1]
    # nine prefixes at one position, the longest of 256 characters: it has no place in either buffer (the character count is a byte)
    parts_long = make_parts([("あ" * n, 1) for n in range(1, 9)] + [("あ" * 256, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=3)
    held_long = Scenario("why2 long key held", parts_long, ["あ" * 255 + "x"], 0)
    handed_long = Scenario("why2 long key handed", parts_long, ["あ" * 256 + "x"], 2)
    (sh,) = held_long.shapes()
    assert max(len(p) for p in sh.prefixes) == WMAXM and sh.parked(0) == 0
    (sh,) = handed_long.shapes()
    assert len(sh.prefixes[0]) == WMAXM + 1 and sh.prefixes[0][-1][0] == 256 and sh.parked(0) == 1
    return [held, handed, held_long, handed_long]


def scenarios_why8():
    """why 8: a window that does not fit the LDS even four positions long.  A node costs at least 14 bytes of LDS (8 + 4 + 2: kgpu_window.hip's carve),
    its bucket slot 8 more."""
    dense = make_parts([("あ", 300)], invoke=(0, 1, 1), group=(0, 1, 0), seed=4)
    mild = make_parts([("あ", 20)], invoke=(0, 1, 1), group=(0, 1, 0), seed=4)
    handed = Scenario("why8 handed", dense, ["テスト" + "あ" * 8 + "辞書"], 8)
    held = Scenario("why8 held", mild, ["テスト" + "あ" * 40 + "辞書"], 0)
    (sh,) = handed.shapes()
    assert sh.per_pos[3:11] == [301] * 8 and min(sum(sh.per_pos[i : i + 4]) for i in range(3, 8)) * 14 > WINDOW_LDS_DEFAULT
    (sh,) = held.shapes()
    assert sum(sh.per_pos[3 : 3 + WIN]) * 22 > WINDOW_LDS_DEFAULT    # a full-length window cannot fit: the windows are shortened ...
    assert max(sum(sh.per_pos[i : i + 4]) for i in range(sh.C)) * 30 + 4096 < WINDOW_LDS_DEFAULT   # ... and four positions fit with room to spare
    return [held, handed]


def scenarios_why6():
    """why 6: far entries (nodes longer than NEARLEN characters) whose ends decrease: the FIFO lives on non-decreasing ends."""
    K50 = "漢" * 40 + "あ" * 10   # starts a run of 40 of a group + invoke category: the known end (50) is written before the unknown one (40), in one lane
    parts = make_parts([("あ" * 34, 1), ("あ" * 50, 1), (K50, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=6)
    parts_ok = make_parts([("あ" * 34, 1), ("あ" * 35, 1), ("漢" * 50, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=6)
    handed = Scenario("why6 handed", parts, ["あ" * 52, "x" + K50 + "x"], 6)
    held = Scenario("why6 held", parts_ok, ["あ" * 52, "x" + "漢" * 50 + "x"], 0)
    a, b = handed.shapes()
    assert [e for _, e, _ in a.far()][:3] == [34, 50, 35] and [e for _, e, _ in b.far()][:2] == [51, 41]
    assert not a.far_ends_never_decrease() and not b.far_ends_never_decrease()
    for sh in held.shapes():
        assert len(sh.far()) >= 10 and sh.far_ends_never_decrease()
    return [held, handed]


def scenarios_why1():
    """why 1: a FIFO entry that ends in a window lies more than 0x8000 nodes behind the window's first node.  A run of 1100 digits (group + invoke): the
    unknown word of position 0 is 1024 characters long, and every position in between starts `records + 1` nodes."""
    out = []
    for dup, why in ((20, 0), (40, 1)):
        parts = make_parts([("1", dup)], invoke=(0, 1, 0), group=(0, 1, 0), seed=7, digits_cat=1)
        sc = Scenario("why1 " + ("handed" if why else "held"), parts, ["1" * 1100], why)
        (sh,) = sc.shapes()
        assert sh.per_pos == [dup + 1] * 1100 and sh.nodes_with_bos == 1100 * (dup + 1) + 2
        gaps = sh.seed_gaps()
        lo, hi = sh.fifo_waiting()
        assert len(gaps) == 1100 - NEARLEN and hi.max() < FIFO_LIMIT and sh.nodes_with_bos < NODE_LIMIT and sh.far_ends_never_decrease()
        if why:
            assert gaps[0][0] == (1024 - WIN + 1) * 41 - 40 > REBASE    # the first entry that ends at all (position 0's, at 1024): too far behind wherever the window starts
        else:
            assert max(g for _, g in gaps) == 1024 * 21 - 20 < REBASE   # about 21.5 k nodes at the most
        out.append(sc)
    return out


def scenarios_why4():
    """why 4: more far entries waiting than the FIFO's chunks hold.  A group category with many unknown records: every position of a run adds that many
    entries, and all of them end where the run ends.  The last WIN positions of such a run add near entries with that same end, which the windows in
    front of that end carry along: up to 32 x records of them, in 17 bytes of LDS each -- or in the team's carry bank of CCAP.  At the default 10 KB
    (windows of a few positions) no sentence with more than about eleven such records per position is HELD, whatever its FIFO does (window_handed[8];
    [7] in the team form), so a held twin anywhere near 61440 waiting entries needs a larger window: the pair runs at KGPU_WINDOW=64, where no window is
    shortened and the boundaries are the multiples of WIN.  A run of 700 then carries 4 positions' entries into its last window and both forms hold it;
    a run of 704 ends ON a boundary, all 32 x 40 entries are carried, and the team hands it to the ordinary form (why 7), which holds it.  The last
    scenario overflows the FIFO at the default window: 63 records are about the most four positions fit there, a run cannot be longer than
    MAX_UNKNOWN_LEN, and why 1 stays quiet only because nothing ends before the FIFO is full."""
    env = {"KGPU_WINDOW": "64"}
    roomy = make_parts([("テスト", 1)], unk=(1, 40, 1), seed=8)
    fits = Scenario("why4 held", roomy, ["漢" * 700], 0, env=env, lds=64 * 1024)
    fits_team7 = Scenario("why4 held, the run ends on a window boundary", roomy, ["漢" * 704], 0, env=env, lds=64 * 1024, team_why=7)
    full = Scenario("why4 handed", make_parts([("テスト", 1)], unk=(1, 80, 1), seed=8), ["漢" * 900], 4, env=env, lds=64 * 1024)
    full10 = Scenario("why4 handed, default window", make_parts([("テスト", 1)], unk=(1, 63, 1), seed=8), ["漢" * 1024], 4)
    for sc, m, L in ((full, 80, 900), (full10, 63, 1024)):
        (sh,) = sc.shapes()
        lo, hi = sh.fifo_waiting()
        p4 = int(np.argmax(lo > FIFO_LIMIT))             # the window that holds this position overflows the FIFO, if none before it did
        longest = min(WIN, sc.lds // (14 * m))           # positions of a window at this density (14 bytes of LDS per node at the least)
        assert lo.max() == m * (L - NEARLEN) > FIFO_LIMIT and lo[p4] > FIFO_LIMIT
        assert min(e for _, e, _ in sh.far()) >= p4 + longest     # nothing ends in any window up to that one: no seed is looked at (why 1), nothing leaves the FIFO
        assert max(sh.carried(b) for b in range(1, p4 + longest + 1)) <= 1   # ... and nothing to speak of is carried (why 7 in the team form)
    assert WIN * 40 * 30 * 8 < 7 * (64 * 1024 - 4096)   # a full window of the twins takes well under 7/8 of 64 KB (30 bytes a node, far slot included): none is shortened
    for sc, L, at_most in ((fits, 700, 4 * 40), (fits_team7, 704, WIN * 40)):
        (sh,) = sc.shapes()
        lo, hi = sh.fifo_waiting()
        assert hi.max() == 40 * (L - NEARLEN) < FIFO_LIMIT and sh.nodes_with_bos == L * 40 + 2 < REBASE   # (fewer than 0x8000 nodes in all: why 1 cannot fire)
        assert max(sh.carried(b) for b in range(WIN, L + 1, WIN)) == at_most and (at_most > CCAP) == (sc.team_why == 7)
        assert sh.carried(L - 1) * 17 > WINDOW_LDS_DEFAULT   # what a 10 KB window in front of the run's end would have to carry
    return [fits, fits_team7, full, full10]


def scenarios_why3():
    """why 3: 262144 nodes in one sentence (BOS included).  あ with 30 records: 30 nodes per character, one for every x, one for EOS, one for BOS."""
    parts = make_parts([("あ", 30)], invoke=(0, 1, 0), group=(0, 1, 0), seed=9)
    L = (NODE_LIMIT - 3) // 30
    held = Scenario("why3 held", parts, ["あ" * L + "x" * (NODE_LIMIT - 3 - 30 * L)], 0)
    handed = Scenario("why3 handed", parts, ["あ" * L + "x" * (NODE_LIMIT - 2 - 30 * L)], 3)
    assert [sh.nodes_with_bos for sh in held.shapes()] == [NODE_LIMIT - 1] and [sh.nodes_with_bos for sh in handed.shapes()] == [NODE_LIMIT]
    assert len(handed.sentences[0]) == len(held.sentences[0]) + 1 < 8800
    return [held, handed]


def scenarios_why7():
    """why 7 (TEAM form only): a carry list beyond CCAP entries.  Keys of 1, 8, 16, 24 and 32 characters (five prefixes per position, none parked):
    1 + 8 + 16 + 24 + 32 = 81 nodes per record reach across any position of a run.  The ordinary form behind the team holds the sentence."""
    env = {"KGPU_WINDOW": "24"}
    out = []
    for dup, why in ((4, 0), (8, 7)):
        parts = make_parts([("あ" * n, dup) for n in (1, 8, 16, 24, 32)], invoke=(0, 1, 0), group=(0, 1, 0), seed=10)
        sc = Scenario("why7 " + ("handed" if why else "held"), parts, ["あ" * 100 + "x"], 0, env=env, lds=24 * 1024, team_why=why)
        (sh,) = sc.shapes()
        assert max(len(p) for p in sh.prefixes) == 5 <= WMAXM and not sh.far()
        carried = [sh.carried(b) for b in range(1, sh.C + 1)]
        if sc.team_why:   # window boundaries are at most WIN apart: one of them falls in [16, 48), whatever the windows' lengths
            assert min(carried[15:47]) == 57 * dup > CCAP and max(carried) == 81 * dup
        else:
            assert max(carried) == 81 * dup <= CCAP
        out.append(sc)
    return out


ALL_SCENARIOS = [scenarios_why1, scenarios_why2, scenarios_why3, scenarios_why4, scenarios_why6, scenarios_why7, scenarios_why8]


def arena_batches():
    """Two batches of 64 sentences of about 400 characters over a small dictionary with digits as a group + invoke category: every sentence needs a
    node chunk of 96 KB (and a slab), the second batch's 200-digit runs far chunks of 64 KB as well -- several times a scratch arena of 1 MiB."""
    parts = make_parts([("テスト", 2), ("辞書", 1), ("形態素", 3), ("あい", 1), ("1", 2)], invoke=(0, 1, 1), group=(0, 1, 1), seed=11, digits_cat=1)
    rng = np.random.default_rng(12)
    pieces = ["テスト", "辞書", "形態素", "あいう", "かな", "xyz", "漢字", "12"]
    plain = ["".join(rng.choice(pieces, size=200))[:400] for _ in range(64)]
    digits = [s[:100] + "1" * 200 + s[100:200] for s in plain]
    assert all(len(s) == 400 for s in plain + digits)
    return parts, plain, digits


# ---------------------------------------------------------------------------------------------------------------- the GPU side
@pytest.fixture(scope="module")
def libs():
    from kanpyo_amd import _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    from oracle import oracle

    oracle.build()
    return _lib, oracle


ROUTING_KEYS = ("deferred", "redone", "window_handed", "tail_reruns", "arena_regrows", "window_reruns", "long_launches")


def run_batch(ctx, orc, sentences, exp=None):
    """One batch through the device API on `ctx`: records, offsets and status must be the oracle's.  -> (routing counters of this batch, oracle result)."""
    import torch

    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sentences)
    if exp is None:
        exp = orc.tokenize_batch(utf8, offs, 8)
    dev = torch.device("cuda", 0)
    n, cap = len(sentences), int(offs[-1]) + len(sentences)
    d_utf8 = torch.from_numpy(utf8.copy()).to(dev) if utf8.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
    nt = ctx.sync()
    status, toff, t = d_st.cpu().numpy(), d_toff.cpu().numpy().astype(np.uint64), d_tok[:nt].cpu().numpy().reshape(-1)
    assert not status.any(), status.nonzero()
    assert np.array_equal(toff, exp.offsets), "per-sentence token counts differ"
    want = exp.tokens.view(np.int32).reshape(-1)
    if not np.array_equal(t, want):
        bad = int(np.nonzero(t != want)[0][0]) // 6
        s = int(np.searchsorted(exp.offsets, bad, side="right") - 1)
        raise AssertionError(f"token {bad} (sentence {s}, {len(sentences[s])} characters) differs: gpu {t[6 * bad : 6 * bad + 6]} oracle {exp.tokens[bad]}")
    p = ctx.profile(reset=True)
    return {k: p[k] for k in ROUTING_KEYS}, exp


def run_scenario(sc, team, monkeypatch):
    """The scenario's sentences one by one between ordinary ones (their own workgroups in a batch this small; test_the_next_sentence_of_a_workgroup puts
    a workgroup's next sentence behind a handed one), each batch twice on one context."""
    from kanpyo_amd import Tokenizer
    from kanpyo_amd.device import DeviceContext

    orc = sc.oracle()
    monkeypatch.setenv("KGPU_POOL", "0")
    monkeypatch.setenv("KGPU_WINDOW_TEAM", "2" if team else "0")
    monkeypatch.delenv("KGPU_WINDOW", raising=False)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    tok = Tokenizer(sc.dict)
    ctx = DeviceContext(tok)
    assert ctx.plan()["window_lds_bytes"] == sc.lds
    for special in sc.sentences:
        batch = ORDINARY[:3] + [special] + ORDINARY[3:] + [special] + ORDINARY[:2]
        first, exp = run_batch(ctx, orc, batch)
        again, _ = run_batch(ctx, orc, batch, exp)
        assert first == again, (sc.name, first, again)
        print(f"{sc.name} ({'team' if team else 'ordinary'} form), {len(special)} characters x 2: {first}")
        zero, want = [0] * 10, [0] * 4   # (every special sentence is in the batch twice)
        if team and sc.team_why:         # the team hands them to the ordinary form behind it (list 0) ...
            zero[sc.team_why] += 2
            want[0] = 2
        if sc.why:                       # ... which hands them on as well (list 1 then), or is the only form (list 0)
            zero[sc.why] += 2
            want[1 if team else 0] = 2
        assert first["window_handed"] == zero and first["deferred"] == want, (sc.name, team, first)
        assert first["window_reruns"] == 0 and first["arena_regrows"] == 0 and first["tail_reruns"] == (1 if want[1 if team else 0] else 0), (sc.name, first)   # (the chain ends on list 1 behind the team, on list 0 without)
    ctx.close()
    tok.close()


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
