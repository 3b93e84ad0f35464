"""The lattice sweep's cases reach what they claim (tests/lattice_cases.py; tests/test_gpu_lattice_sweep.py runs them on the device): every crafted
shape of the catalogue is present by its own measure, and the seeded generators give the mixes and the widths the sweep relies on.  Everything is
read off the naive restatement's lattice (oracle/pyref.py) and, for the user dictionary, off tests/userdict_ref.widen: no call that needs a device,
and a generator someone weakens later fails here.  The counts asserted are floors; what the seeds give is printed."""
import pytest

import lattice_cases as L
import userdict_ref as R
from dict_cases import lattice_from_pyref
from oracle import pyref

INF = 1 << 30


@pytest.fixture(scope="module")
def shapes():
    """{case name: [Shape per sentence]} of the catalogue, measured once."""
    out = {}
    for case in L.catalogue():
        pd = L.pydict_of(case.make())
        out[case.name] = [L.shape_of(pd, s) for s in case.sentences]
    return out


def test_every_claim_of_the_catalogue_holds(shapes):
    for case in L.catalogue():
        assert case.claims, case.name
        for i, claim in case.claims:
            assert L.holds(shapes[case.name][i], claim), (case.name, i, claim)


def test_named_shapes(shapes):
    """The shapes the sweep was written for, by name: a catalogue that loses one of them fails here, whatever its own claims say."""
    assert sorted(shapes) == sorted(["parked matches", "keys of 255 and 256 characters", "chunk pairing", "unknown length cap", "sweep step", "unreachable predecessor",
                                     "characters, short category table", "characters, full category table"])
    sh = shapes["parked matches"]
    assert any(a == 9 and b == 8 for s in sh for a, b in zip(s.matches, s.matches[1:]))                      # GMAXM: 9 matches, then exactly 8
    assert any(s.matches[63:65] == [9, 8] for s in sh if s.C > 64)                                           # ... in two chunks as well
    sh = shapes["keys of 255 and 256 characters"]
    assert any((m, n) == (8, 255) for s in sh for m, n in zip(s.matches, s.longest))                         # nch < 256: parked
    assert any((m, n) == (9, 256) for s in sh for m, n in zip(s.matches, s.longest))
    sh = shapes["chunk pairing"]
    assert sorted({s.C for s in sh}) == list(L.CHUNK_LENGTHS)
    spans = {(s.C, a, b) for s in sh for a, b in s.unknown}
    for C in L.CHUNK_LENGTHS:
        if C > 64:
            assert (C, 60, min(67, C)) in spans and (C, 50, 64) in spans                                          # across 63|64; an end exactly at 64
        if C > 128:
            assert {(C, 125, min(131, C)), (C, 60, min(131, C)), (C, 64, min(131, C))} <= spans             # across 127|128; chunk 1 has no change inside
        assert (C, 0, C) in spans                                                                            # every chunk carries its run end
    lengths = {b - a for s in shapes["unknown length cap"] for a, b in s.unknown}
    assert {1023, 1024} <= lengths and max(lengths) == 1024 and [s.C for s in shapes["unknown length cap"]] == [1025, 1026, 1027]
    sh = shapes["sweep step"]
    pt = {(p, t) for s in sh for p, t in zip(s.P, s.T)}
    assert {47, 48, 64, 65, 129} <= {p for p, _ in pt}
    assert {(p, t) for p, t in pt if p < 48 and t in (64, 65)} >= {(5, 64), (5, 65), (47, 65)}
    for s in sh:                                                                                             # a tie among three or more at every named width
        assert any(s.P[q] in (47, 48, 64, 65, 129) or s.T[q] in (64, 65) for q in s.ties), (s.P, s.T, s.ties)
    sh = shapes["unreachable predecessor"]
    assert sum(bool(s.quirk) for s in sh) >= 2 and sum(not s.reachable for s in sh) >= 3
    for name in ("characters, short category table", "characters, full category table"):
        assert shapes[name][0].C == 0 and shapes[name][0].reachable and shapes[name][0].P == [1, 1]          # "": BOS and EOS


def test_the_tables_length_decides_a_category():
    """漢 U+FFFF and a non-BMP character in a row: one run of table[0]'s category where the table ends before them, three categories where it does not."""
    short, full = (L.pydict_of(L.chars_dict(n)) for n in (0x3100, 65536))
    s = L.CHAR_SENTENCES[6]
    assert [short.char_category(ord(c)) for c in s] == [0, 2, 2, 2, 0] and [full.char_category(ord(c)) for c in s] == [0, 0, 2, 1, 0]


def _mix(gen, count_matches=False):
    """-> counts over a sweep: sentences, with a reachable EOS, with a node behind an unreachable predecessor, panics, the widest P and T, and on
    request the most trie matches at a position."""
    n = reach = quirk = panic = maxp = maxt = most = 0
    for _, d, sents in gen:
        pd = L.pydict_of(d)
        for s in sents:
            n += 1
            try:
                nodes, edges, dp, pre = pyref.lattice(pd, s)
            except pyref.Panic:
                panic += 1
                continue
            reach += pre[-1] is not None
            quirk += any(pre[i] is not None and dp[i] < INF and dp[pre[i]] == INF for i in range(1, len(nodes)))
            t = {}
            for x in nodes[1:]:
                t[x[3]] = t.get(x[3], 0) + 1
            maxp, maxt = max(maxp, max(len(e) for e in edges)), max(maxt, max(t.values()))
            if count_matches:
                raw, b = s.encode("utf-8"), 0
                for ch in s:
                    most = max(most, len(pd.da_common_prefix(raw[b:]) or []))
                    b += len(ch.encode("utf-8"))
    return dict(sentences=n, reachable=reach, quirk=quirk, panics=panic, P=maxp, T=maxt, matches=most)


@pytest.mark.parametrize("seed", L.RANDOM_SEEDS)
def test_random_dictionaries_mix(seed):
    m = _mix(L.random_sweep(seed))
    print(f"random sweep, seed {seed}: {m}")
    assert m["sentences"] == 2400 and m["panics"] == 0
    assert m["reachable"] >= 1200 and m["sentences"] - m["reachable"] >= 200 and m["quirk"] >= 200, m


def test_dense_and_width_sweeps_reach_the_wide_steps():
    dense = [_mix(L.dense_sweep(seed), True) for seed in L.DENSE_SEEDS]
    width = [_mix(L.width_sweep(seed), True) for seed in L.WIDTH_SEEDS]
    print(f"dense sweeps {dict(zip(L.DENSE_SEEDS, dense))}\nwidth sweeps {dict(zip(L.WIDTH_SEEDS, width))}")
    assert all(m["panics"] == 0 and m["sentences"] >= 300 for m in dense + width)
    assert max(m["P"] for m in dense) > 128 and max(m["T"] for m in dense) > 64, dense
    assert max(m["matches"] for m in dense + width) < 8   # never GMAXM matches at a position, let alone nine: why the parked-match cases are crafted


def test_user_cases_decide_what_they_name():
    for case in L.user_cases():
        d = case.make()
        lat = lattice_from_pyref(L.pydict_of(d), case.sentence)
        got = L.user_decisions(lat, case.sentence, case.entries, R.invoke_of(d, case.sentence))
        assert got == (case.withdrawn, case.kept_by_invoke), (case.name, got)
    # the twins differ in their invoke bit alone
    d = L.twin_dict()
    pd = L.pydict_of(d)
    assert pd.invoke[1:] == [False, True] and pd.group[1] == pd.group[2] and [pd.unk_morphs[pd.unk[c][0] - 1] for c in (1, 2)] == [(1, 1, 3000)] * 2


@pytest.mark.parametrize("seed", L.RANDOM_SEEDS)
def test_user_sweep_withdraws_and_keeps(seed):
    withdrawn = kept = sentences = 0
    for _, d, sents, entries in L.user_sweep(seed):
        pd = L.pydict_of(d)
        assert entries and all(0 <= e[1] < L.contexts_of(d) and 0 <= e[2] < L.contexts_of(d) for e in entries)
        for s in sents:
            a, b = L.user_decisions(lattice_from_pyref(pd, s), s, entries, R.invoke_of(d, s))
            withdrawn, kept, sentences = withdrawn + len(a), kept + len(b), sentences + 1
    print(f"user sweep, seed {seed}: {sentences} sentences, {withdrawn} positions withdrawn, {kept} kept because the category invokes")
    assert sentences == 2400 and withdrawn >= 50 and kept >= 50
