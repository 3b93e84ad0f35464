"""The windowed kernel's constants (kanpyo_amd/csrc/kgpu_window.hip), the tiny-dictionary builder, the plain-Python model of a lattice's shape and
the HELD / HANDED pairs chosen with it for every hand-on limit: what tests/test_gpu_window_limits.py asks the device about, decided BEFORE the
GPU is touched.  The model takes the nodes per start position from the key list, the category table and the unknown-word rules of
src/lattice.rs:42-99, and its node total must equal the oracle's (counters["N"]) for every sentence: the scenarios_* functions assert that while
they build the cases, and tests/test_window_limits_cpu.py runs them without a device.  tests/pool_cases.py builds its dictionaries and shapes with
make_parts and Shape.  Nothing here needs a device or the GPU library at import."""
import numpy as np

from conftest import fixture_dict_parts

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
    assert [sh.parked(0) for sh in held.shapes()] == [XMAX - 1, XMAX], [sh.parked(0) for sh in held.shapes()]
    assert all(max(sh.parked(w) for w in range(0, sh.C, WIN)) <= XMAX for sh in held.shapes()), [[sh.parked(w) for w in range(0, sh.C, WIN)] for sh in held.shapes()]
    assert [sh.parked(0) for sh in handed.shapes()] == [XMAX + 1, XMAX + 1], [sh.parked(0) for sh in handed.shapes()]
    # nine prefixes at one position, the longest of 256 characters: it has no place in either buffer (the character count is a byte)
    parts_long = make_parts([("あ" * n, 1) for n in range(1, 9)] + [("あ" * 256, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=3)
    held_long = Scenario("why2 long key held", parts_long, ["あ" * 255 + "x"], 0)
    handed_long = Scenario("why2 long key handed", parts_long, ["あ" * 256 + "x"], 2)
    (sh,) = held_long.shapes()
    assert max(len(p) for p in sh.prefixes) == WMAXM and sh.parked(0) == 0, ([len(p) for p in sh.prefixes][:4], sh.parked(0))
    (sh,) = handed_long.shapes()
    assert len(sh.prefixes[0]) == WMAXM + 1 and sh.prefixes[0][-1][0] == 256 and sh.parked(0) == 1, (sh.prefixes[0], sh.parked(0))
    return [held, handed, held_long, handed_long]


def scenarios_why8():
    """why 8: a window that does not fit the LDS even four positions long.  A node costs at least 14 bytes of LDS (8 + 4 + 2: kgpu_window.hip's carve),
    its bucket slot 8 more."""
    dense = make_parts([("あ", 300)], invoke=(0, 1, 1), group=(0, 1, 0), seed=4)
    mild = make_parts([("あ", 20)], invoke=(0, 1, 1), group=(0, 1, 0), seed=4)
    handed = Scenario("why8 handed", dense, ["テスト" + "あ" * 8 + "辞書"], 8)
    held = Scenario("why8 held", mild, ["テスト" + "あ" * 40 + "辞書"], 0)
    (sh,) = handed.shapes()
    assert sh.per_pos[3:11] == [301] * 8 and min(sum(sh.per_pos[i : i + 4]) for i in range(3, 8)) * 14 > WINDOW_LDS_DEFAULT, sh.per_pos[:12]
    (sh,) = held.shapes()
    assert sum(sh.per_pos[3 : 3 + WIN]) * 22 > WINDOW_LDS_DEFAULT, sum(sh.per_pos[3 : 3 + WIN])    # a full-length window cannot fit: the windows are shortened ...
    assert max(sum(sh.per_pos[i : i + 4]) for i in range(sh.C)) * 30 + 4096 < WINDOW_LDS_DEFAULT, max(sum(sh.per_pos[i : i + 4]) for i in range(sh.C))   # ... and four positions fit with room to spare
    return [held, handed]


def scenarios_why6():
    """why 6: far entries (nodes longer than NEARLEN characters) whose ends decrease: the FIFO lives on non-decreasing ends."""
    K50 = "漢" * 40 + "あ" * 10   # starts a run of 40 of a group + invoke category: the known end (50) is written before the unknown one (40), in one lane
    parts = make_parts([("あ" * 34, 1), ("あ" * 50, 1), (K50, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=6)
    parts_ok = make_parts([("あ" * 34, 1), ("あ" * 35, 1), ("漢" * 50, 1)], invoke=(0, 1, 0), group=(0, 1, 0), seed=6)
    handed = Scenario("why6 handed", parts, ["あ" * 52, "x" + K50 + "x"], 6)
    held = Scenario("why6 held", parts_ok, ["あ" * 52, "x" + "漢" * 50 + "x"], 0)
    a, b = handed.shapes()
    assert [e for _, e, _ in a.far()][:3] == [34, 50, 35] and [e for _, e, _ in b.far()][:2] == [51, 41], (a.far()[:3], b.far()[:2])
    assert not a.far_ends_never_decrease() and not b.far_ends_never_decrease(), ([e for _, e, _ in a.far()][:8], [e for _, e, _ in b.far()][:8])
    for sh in held.shapes():
        assert len(sh.far()) >= 10 and sh.far_ends_never_decrease(), (len(sh.far()), [e for _, e, _ in sh.far()][:8])
    return [held, handed]


def scenarios_why1():
    """why 1: a FIFO entry that ends in a window lies more than 0x8000 nodes behind the window's first node.  A run of 1100 digits (group + invoke): the
    unknown word of position 0 is 1024 characters long, and every position in between starts `records + 1` nodes."""
    out = []
    for dup, why in ((20, 0), (40, 1)):
        parts = make_parts([("1", dup)], invoke=(0, 1, 0), group=(0, 1, 0), seed=7, digits_cat=1)
        sc = Scenario("why1 " + ("handed" if why else "held"), parts, ["1" * 1100], why)
        (sh,) = sc.shapes()
        assert sh.per_pos == [dup + 1] * 1100 and sh.nodes_with_bos == 1100 * (dup + 1) + 2, (sorted(set(sh.per_pos)), sh.nodes_with_bos)
        gaps = sh.seed_gaps()
        lo, hi = sh.fifo_waiting()
        assert len(gaps) == 1100 - NEARLEN and hi.max() < FIFO_LIMIT and sh.nodes_with_bos < NODE_LIMIT and sh.far_ends_never_decrease(), (len(gaps), int(hi.max()), sh.nodes_with_bos)
        if why:
            assert gaps[0][0] == (1024 - WIN + 1) * 41 - 40 > REBASE, gaps[0]    # the first entry that ends at all (position 0's, at 1024): too far behind wherever the window starts
        else:
            assert max(g for _, g in gaps) == 1024 * 21 - 20 < REBASE, max(g for _, g in gaps)   # about 21.5 k nodes at the most
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
        assert lo.max() == m * (L - NEARLEN) > FIFO_LIMIT and lo[p4] > FIFO_LIMIT, (int(lo.max()), p4, int(lo[p4]))
        assert min(e for _, e, _ in sh.far()) >= p4 + longest, (min(e for _, e, _ in sh.far()), p4, longest)     # nothing ends in any window up to that one: no seed is looked at (why 1), nothing leaves the FIFO
        assert max(sh.carried(b) for b in range(1, p4 + longest + 1)) <= 1, max(sh.carried(b) for b in range(1, p4 + longest + 1))   # ... and nothing to speak of is carried (why 7 in the team form)
    assert WIN * 40 * 30 * 8 < 7 * (64 * 1024 - 4096)   # a full window of the twins takes well under 7/8 of 64 KB (30 bytes a node, far slot included): none is shortened
    for sc, L, at_most in ((fits, 700, 4 * 40), (fits_team7, 704, WIN * 40)):
        (sh,) = sc.shapes()
        lo, hi = sh.fifo_waiting()
        assert hi.max() == 40 * (L - NEARLEN) < FIFO_LIMIT and sh.nodes_with_bos == L * 40 + 2 < REBASE, (int(hi.max()), sh.nodes_with_bos)   # (fewer than 0x8000 nodes in all: why 1 cannot fire)
        assert max(sh.carried(b) for b in range(WIN, L + 1, WIN)) == at_most and (at_most > CCAP) == (sc.team_why == 7), (max(sh.carried(b) for b in range(WIN, L + 1, WIN)), at_most, sc.team_why)
        assert sh.carried(L - 1) * 17 > WINDOW_LDS_DEFAULT, sh.carried(L - 1)   # what a 10 KB window in front of the run's end would have to carry
    return [fits, fits_team7, full, full10]


def scenarios_why3():
    """why 3: 262144 nodes in one sentence (BOS included).  あ with 30 records: 30 nodes per character, one for every x, one for EOS, one for BOS."""
    parts = make_parts([("あ", 30)], invoke=(0, 1, 0), group=(0, 1, 0), seed=9)
    L = (NODE_LIMIT - 3) // 30
    held = Scenario("why3 held", parts, ["あ" * L + "x" * (NODE_LIMIT - 3 - 30 * L)], 0)
    handed = Scenario("why3 handed", parts, ["あ" * L + "x" * (NODE_LIMIT - 2 - 30 * L)], 3)
    assert [sh.nodes_with_bos for sh in held.shapes()] == [NODE_LIMIT - 1] and [sh.nodes_with_bos for sh in handed.shapes()] == [NODE_LIMIT], ([sh.nodes_with_bos for sh in held.shapes()], [sh.nodes_with_bos for sh in handed.shapes()])
    assert len(handed.sentences[0]) == len(held.sentences[0]) + 1 < 8800, (len(handed.sentences[0]), len(held.sentences[0]))
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
        assert max(len(p) for p in sh.prefixes) == 5 <= WMAXM and not sh.far(), (max(len(p) for p in sh.prefixes), len(sh.far()))
        carried = [sh.carried(b) for b in range(1, sh.C + 1)]
        if sc.team_why:   # window boundaries are at most WIN apart: one of them falls in [16, 48), whatever the windows' lengths
            assert min(carried[15:47]) == 57 * dup > CCAP and max(carried) == 81 * dup, (min(carried[15:47]), max(carried), dup)
        else:
            assert max(carried) == 81 * dup <= CCAP, (max(carried), dup)
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
    assert all(len(s) == 400 for s in plain + digits), sorted({len(s) for s in plain + digits})
    return parts, plain, digits
