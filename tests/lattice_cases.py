"""The dictionaries and sentences of the lattice sweep (tests/test_lattice_cases_cpu.py, tests/test_gpu_lattice_sweep.py; tests/test_oracle_fuzz.py
draws its random dictionaries here): the seeded generators, a catalogue of crafted (dictionary, sentences) pairs -- each the smallest shape at which
one statement of k_tokenize_general (kanpyo_amd/csrc/kgpu_kernels.hip) can go wrong, named in a comment -- the user-dictionary cases, and the
measures a lattice of the naive restatement (oracle/pyref.py) is read by: trie matches per position, predecessors (P) and targets (T) per position,
unknown spans, nodes behind an unreachable predecessor, ties that went to the lowest index.  Every claim of the catalogue is stated as data and
checked against those measures on the CPU.  Imports without a device."""
import random
from collections import namedtuple

import numpy as np

from nbest_cases import pydict_of  # noqa: F401  (the one PyDict maker of the case modules)

INF = 1 << 30

# ---- the seeded generators ------------------------------------------------------------------------------------------------------------------------------------
ALPHABETS = [
    "あいうえお", "アイウエオカ", "日本語辞書形態素", "abcXYZ", "0123", "、。 ", "\U00020000\U0002A6D6",  # non-BMP -> category of table[0]
]


def _random_dict(rng, n_cat):
    from kanpyo_amd.dict import Dict

    alpha = "".join(ALPHABETS)
    n_words = int(rng.integers(1, 60))
    words = set()
    while len(words) < n_words:
        src = rng.choice(len(ALPHABETS))
        w = "".join(rng.choice(list(ALPHABETS[src]), size=int(rng.integers(1, 5))))
        words.add(w)
        if rng.random() < 0.4 and len(w) < 6:  # nested prefix
            words.add(w + str(rng.choice(list(alpha))))
    records = []
    for w in sorted(words, key=lambda s: s.encode("utf-8")):
        for _ in range(int(rng.choice([1, 1, 1, 2, 3, 6]))):  # duplicate surfaces
            records.append(w)
    n_ctx = int(rng.integers(1, 7))
    morphs = np.stack([rng.integers(0, n_ctx, len(records)), rng.integers(0, n_ctx, len(records)),
                       rng.integers(-3000, 9000, len(records))], axis=1)
    matrix = rng.integers(-4000, 4000, size=n_ctx * n_ctx)
    cat = np.zeros(65536, dtype=np.uint8)
    for k, a in enumerate(ALPHABETS[:-1]):
        for ch in a:
            cat[ord(ch)] = k % n_cat
    invoke = rng.integers(0, 2, n_cat).astype(np.uint8)
    group = rng.integers(0, 2, n_cat).astype(np.uint8)
    unk_map, unk_morphs, nxt = {}, [], 1
    for c in range(n_cat):
        if rng.random() < 0.75:  # some categories have no unk entry: dead ends, unreachable EOS
            cnt = int(rng.integers(1, 4))
            unk_map[c] = (nxt, cnt)
            for _ in range(cnt):
                unk_morphs.append((int(rng.integers(0, n_ctx)), int(rng.integers(0, n_ctx)), int(rng.integers(-2000, 12000))))
            nxt += cnt
    return Dict.from_parts(records, morphs, n_ctx, n_ctx, matrix, [f"C{c}" for c in range(n_cat)], cat, invoke, group, unk_map, unk_morphs)


def _sentence(rng):
    parts = []
    for _ in range(int(rng.integers(0, 7))):
        a = ALPHABETS[int(rng.integers(0, len(ALPHABETS)))]
        parts.append("".join(rng.choice(list(a), size=int(rng.integers(1, 6)))))
    return "".join(parts)


# ---- the sweeps: (what, Dict, sentences) per dictionary, seeded -----------------------------------------------------------------------------------------------------
RANDOM_SEEDS = (101, 102)              # 60 dictionaries x 40 sentences each
DENSE_SEEDS = (9001, 4242, 777, 31337)  # tests/test_gpu_fuzz.py's: 12 dictionaries each, their first 64 sentences
WIDTH_SEEDS = (20260929, 1234)
USER_COSTS = (-1500, 0, 2500)


def random_sweep(seed: int):
    rng = np.random.default_rng(seed)
    for k in range(60):
        d = _random_dict(rng, int(rng.integers(1, 6)))
        yield f"random seed {seed} dictionary {k}", d, [_sentence(rng) for _ in range(40)]


def _synth_sweep(name: str, seed: int):
    from kanpyo_amd import synth

    rng = random.Random(seed)
    for k in range(12):
        d, sents = getattr(synth, name)(rng)
        yield f"{name} seed {seed} dictionary {k}", d, sents[:64]


def dense_sweep(seed: int):
    return _synth_sweep("dense_case", seed)


def width_sweep(seed: int):
    return _synth_sweep("width_case", seed)


def contexts_of(d) -> int:
    """The context ids a user entry may carry: below both axes of the dictionary's matrix."""
    rows, cols = d.conn_shape
    return int(min(rows, cols))


def user_sweep(seed: int):
    """random_sweep with entries cut from each dictionary's first sentences (userdict_cases.entries_from) -> (what, Dict, sentences, entries)."""
    from userdict_cases import entries_from

    rng = random.Random(seed * 7 + 3)
    for what, d, sents in random_sweep(seed):
        entries = [e for s in [s for s in sents if s][:8] for e in entries_from(rng, s, 2, USER_COSTS, nctx=contexts_of(d))]
        yield what, d, sents, entries


# ---- measures over pyref.lattice ---------------------------------------------------------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "C matches longest P T unknown quirk ties reachable")


def shape_of(pd, text: str, lat=None) -> Shape:
    """What a lattice of the restatement shows, by its own measure: matches[q] the keys that are a prefix of the text at q (the trie's, before duplicate
    records) and longest[q] the longest of them in characters; P[q] the nodes that end at q, T[q] those that start there (EOS at C); unknown the
    (start, end) of every unknown node; quirk the nodes with dp < 1 << 30 whose predecessor's dp is 1 << 30; ties the start positions of the nodes whose best total three
    or more predecessors share, the lowest index among them chosen; reachable: EOS has a predecessor."""
    from oracle import pyref

    nodes, edges, dp, pre = lat if lat is not None else pyref.lattice(pd, text)
    C = len(text)
    raw = text.encode("utf-8")
    matches, longest, b = [], [], 0
    for ch in text:
        r = pd.da_common_prefix(raw[b:]) or []
        matches.append(len(r))
        longest.append(max((len(raw[b : b + n].decode("utf-8")) for _, n in r), default=0))
        b += len(ch.encode("utf-8"))
    T = [0] * (C + 1)
    for n in nodes[1:]:
        T[n[3]] += 1
    unknown = {(n[3], n[3] + n[6]) for n in nodes if n[0] == 2}
    quirk = [i for i in range(1, len(nodes)) if pre[i] is not None and dp[i] < INF and dp[pre[i]] == INF]
    ties = set()
    for i in range(1, len(nodes)):
        if pre[i] is None:
            continue
        t = nodes[i]
        same = [j for j in edges[t[3]] if min((dp[j] or 0) + t[4][2] + pd.conn[pd.row * t[4][0] + nodes[j][4][1]], INF) == dp[i]]
        if len(same) >= 3 and pre[i] == min(same):
            ties.add(t[3])
    return Shape(C, matches, longest, [len(e) for e in edges], T, unknown, quirk, ties, pre[-1] is not None)


def holds(shape: Shape, claim: tuple) -> bool:
    """One claim of the catalogue against a sentence's Shape."""
    kind, *v = claim
    if kind in ("matches", "longest", "P", "T"):
        return getattr(shape, kind)[v[0]] == v[1]
    if kind == "unknown":
        return (v[0], v[1]) in shape.unknown
    if kind == "no_unknown":      # no unknown node starts at v[0] (or none with this span, where an end is given)
        return not any(s == v[0] and (len(v) == 1 or e == v[1]) for s, e in shape.unknown)
    if kind == "tie":             # a target that starts at v[0] had three or more equal candidates
        return v[0] in shape.ties
    if kind == "quirk":
        return bool(shape.quirk)
    if kind == "reachable":
        return shape.reachable == v[0]
    raise ValueError(kind)


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name make sentences claims")   # claims: [(sentence index, (kind, ...))]
A, X = "あ", "x"


def _build(words, nctx, conn, cat_of, invoke, group, unk, cat_len=65536, cat0=0):
    """Dict.from_parts over words [(surface, left, right, cost)] -- a surface that comes more than once has that many records, in the order given --
    cat_of {character: category}, unk {category: [(left, right, cost)]}, a category table of cat_len entries whose entry 0 is cat0."""
    from kanpyo_amd.dict import Dict

    order = sorted(range(len(words)), key=lambda k: (words[k][0].encode("utf-8"), k))
    cat = np.zeros(cat_len, dtype=np.uint8)
    cat[0] = cat0
    for ch, c in cat_of.items():
        cat[ord(ch)] = c
    unk_map, unk_morphs = {}, []
    for c in sorted(unk):
        unk_map[c] = (len(unk_morphs) + 1, len(unk[c]))
        unk_morphs += list(unk[c])
    return Dict.from_parts([words[k][0] for k in order], np.array([words[k][1:4] for k in order], dtype=np.int64).reshape(-1, 3), nctx, nctx, conn,
                           [f"C{c}" for c in range(len(invoke))], cat, np.array(invoke, dtype=np.uint8), np.array(group, dtype=np.uint8), unk_map, unk_morphs)


CONN3 = [((r * 5 + l * 3) % 7 - 3) * 50 for l in range(3) for r in range(3)]
PARKED_RECORDS = (1, 2, 1, 3, 1, 1, 2, 1, 2)   # records of あ x 1 .. あ x 9


def parked_dict():
    """on_match: `m < GMAXM && nch < 256` parks a match, anything else sets mcnt to 0xFF and the emit phase walks again.  Nested keys あ x 1 .. あ x 9,
    some with duplicate records: nine matches where nine characters are left, eight at the next position."""
    words = [(A * n, (n + r) % 3, (n * 2 + r) % 3, 100 * ((n + r) % 4)) for n in range(1, 10) for r in range(PARKED_RECORDS[n - 1])]
    return _build(words, 3, CONN3, {A: 1}, [0, 1], [1, 1], {0: [(0, 0, 3000)], 1: [(1, 1, 2500)]})


def long_key_dict():
    """on_match: `nch < 256` (mnch is a byte).  Keys あ x 1 .. あ x 7, あ x 255 and あ x 256: eight matches with one of 255 characters fit the parking
    area, the ninth of 256 does not fit twice over."""
    words = [(A * n, n % 3, (n + 1) % 3, 100 * (n % 5)) for n in (1, 2, 3, 4, 5, 6, 7, 255, 256)]
    return _build(words, 3, CONN3, {A: 1}, [0, 1], [1, 1], {0: [(0, 0, 3000)], 1: [(1, 1, 2500)]})


G, G2 = "ア", "イ"
CHUNK_LENGTHS = (63, 64, 65, 127, 128, 129, 192, 193)


def chunk_dict():
    """The count phase: chunks of 64 positions walked two at a time from the back, `run_end = rest ? i + ffs(rest) : carry_end`.  x: default, one
    character a word; ア: grouped and invoking beside its known words; イ: grouped, unknown only where no word starts."""
    words = [(G, 0, 1, 400), (G + G, 1, 0, 500), (G + G, 1, 1, 450), (G + X, 0, 0, 300), (G2 + G2, 1, 1, 200)]
    return _build(words, 2, [0, 30, -20, 10], {G: 1, G2: 2}, [0, 1, 0], [0, 1, 1], {0: [(0, 0, 2000)], 1: [(1, 0, 1500), (0, 1, 1600)], 2: [(1, 1, 1800)]})


def _runs(C: int, runs, fill=X) -> str:
    s = [fill] * C
    for a, b, ch in runs:
        for i in range(a, min(b, C)):
            s[i] = ch
    return "".join(s)


def chunk_sentences():
    """-> (sentences, claims): per C a run across 63|64 and one across 127|128; one that ends exactly at 64; one over a whole chunk and more (no
    category change inside chunk 1: `rest == 0`, the run end is the carried one); the whole sentence one run (every chunk carries); a change of
    grouped category exactly at 64 and at 128; a run from the middle to one short of the end.  Odd chunk counts (C <= 64, 129 .. 192) leave the
    second slot of a round without a chunk."""
    sents, claims = [], []

    def add(s, *spans):
        sents.append(s)
        claims.extend((len(sents) - 1, ("unknown", a, b)) for a, b in spans if a < b)

    for C in CHUNK_LENGTHS:
        add(_runs(C, [(60, 67, G), (125, 131, G)]), (60, min(67, C)), (66, min(67, C)), (125, min(131, C)))
        add(_runs(C, [(50, 64, G)]), (50, min(64, C)), (63, min(64, C)))
        add(_runs(C, [(60, 131, G)]), (60, min(131, C)), (64, min(131, C)), (127, min(131, C)))
        add(_runs(C, [(0, C, G)]), (0, C), (C - 1, C))
        add(_runs(C, [(0, 64, G), (64, 128, G2), (128, C, G)]), (0, min(64, C)), (min(128, C) - 1, min(128, C)) if C > 64 else (0, 0), (128, C))
        add(_runs(C, [(C // 3, C - 1, G)]), (C // 3, C - 1), (C - 1, C))
    return sents, claims


def cap_sentences():
    """`span = r < MAX_UNKNOWN_LEN ? r : MAX_UNKNOWN_LEN`: grouped runs of 1023, 1024 and 1025 characters between ordinary ones."""
    sents = [X + G * n + X for n in (1023, 1024, 1025)]
    return sents, [(0, ("unknown", 1, 1024)), (1, ("unknown", 1, 1025)), (2, ("unknown", 1, 1025)), (2, ("no_unknown", 1, 1026)), (2, ("unknown", 2, 1026)),
                   (2, ("P", 1026, 2 * 1024 + 3))]   # (ア's two unknown records from 1024 positions, the word ア and the two records of アア)


P_CHARS = {47: "あ", 48: "い", 64: "う", 65: "え", 129: "お"}
KA, KE, KO, SA = "か", "け", "こ", "さ"


def sweep_dict():
    """global_step: `P >= 48` takes the form where the lanes share a target and split its predecessors (`j += 64`: a second round at 65, a third at
    129); below, a lane owns a target (`t += 64`: a second round at T = 65).  `e.z < bidx` makes the lowest node index win a tie whatever order the
    atomics filled the bucket in.  か + c ends where c does, so a bucket of P holds nodes of two start positions: P - 7 records of c, 7 of か c.
    Costs 0 but for a few of 100, the first records of か c among them: the winners are neither first in the bucket nor alone."""
    words = [(KA, 0, r % 2, 0) for r in range(5)]
    for P, c in P_CHARS.items():
        words += [(KA + c, 0, r % 2, 100 if r < 2 else 0) for r in range(7)]
        words += [(c, r % 2, (r // 2) % 2, 100 if r % 5 == 0 else 0) for r in range(P - 7)]
    words += [(KE, r % 2, r % 2, 10 * (r % 3)) for r in range(64)] + [(KO, r % 2, (r + 1) % 2, 10 * (r % 4)) for r in range(65)]
    words += [(SA, 0, 0, 5), (SA, 1, 0, 5), (SA, 0, 1, 7)]
    chars = {ch: 1 for ch in list(P_CHARS.values()) + [KA, KE, KO, SA]}
    return _build(words, 2, [0, 50, 50, 0], chars, [0, 0], [1, 0], {0: [(0, 0, 3000)], 1: [(1, 1, 2500)]})


def sweep_sentences():
    sents, claims = [], []
    for P, c in P_CHARS.items():
        sents.append(KA + c + SA)
        claims += [(len(sents) - 1, ("P", 2, P)), (len(sents) - 1, ("T", 2, 3)), (len(sents) - 1, ("tie", 2))]
    for T, c in ((64, KE), (65, KO)):
        sents.append(KA + c)
        claims += [(len(sents) - 1, ("P", 1, 5)), (len(sents) - 1, ("T", 1, T)), (len(sents) - 1, ("tie", 1))]
    for P in (47, 48):   # the widest of both at one position
        sents.append(KA + P_CHARS[P] + KO + SA)
        claims += [(len(sents) - 1, ("P", 2, P)), (len(sents) - 1, ("T", 2, 65)), (len(sents) - 1, ("tie", 2)), (len(sents) - 1, ("P", 3, 65))]
    sents.append(KA + KE + SA + KA + P_CHARS[129] + P_CHARS[65] + SA)
    claims += [(len(sents) - 1, ("P", 2, 64)), (len(sents) - 1, ("P", 5, 129)), (len(sents) - 1, ("P", 6, 65 - 7))]
    return sents, claims


def quirk_dict():
    """The sweep's `tot < INF` after `best + cost`: a predecessor of dp 1 << 30 and a word whose cost plus connection cost is negative give a total
    below 1 << 30 (INF + negative < INF, as in the reference), so the word is reached through a node nothing reaches.  z: a category with no unknown
    entry; y: the default one; あ: a known word of cost -3000."""
    return _build([(A, 1, 1, -3000)], 2, [0, 40, -30, 20], {"z": 1, A: 2}, [0, 0, 0], [0, 0, 0], {0: [(0, 0, 3000)], 2: [(1, 0, 2500)]})


QUIRK_SENTENCES = ["zy" + A, "z", A + "z", "zy" + A + "zy" + A, "yz" + A, "y" + A + "y"]
QUIRK_CLAIMS = [(0, ("quirk",)), (0, ("reachable", True)), (1, ("reachable", False)), (2, ("reachable", False)), (3, ("quirk",)), (4, ("reachable", False)),
                (5, ("reachable", True))]
NB, NB2, FFFF, KAN = "\U00020000", "\U00020001", "\uffff", "漢"
CHAR_SENTENCES = ["", NB + A + X, X + NB, NB + NB + A, FFFF + A + FFFF, A + FFFF + X, X + KAN + NB + FFFF + "y", NB2, X + "\U0010FFFF", KAN + KAN + X + NB + KAN,
                  A + NB2 + A + NB]


def chars_dict(cat_len: int):
    """Phase 0: `code = cp < 0xFFFF ? cp : 0xFFFF` (cp16 keeps 0xFFFF for "not BMP", and U+FFFF itself is a character), the non-BMP fallback of the
    byte-level walk, and `cp < d.cat_len ? d.cat[cp] : d.cat[0]`.  Keys that begin with, hold and end in a character outside the BMP and U+FFFF.  Entry
    0 of the table is category 2 (grouped, invoking): with a table of 0x3100 entries 漢, U+FFFF and every non-BMP character are of it; with one of
    65536, 漢 is of category 0 and U+FFFF of category 1."""
    words = [(NB, 0, 0, 300), (NB + A, 1, 0, 200), (A + NB, 0, 1, 250), (FFFF, 1, 1, 350), (FFFF + A, 0, 0, 150), (A + FFFF, 1, 0, 100), (KAN, 0, 1, 400), (A, 0, 0, 500)]
    cat_of = {A: 1}
    if cat_len > 0xFFFF:
        cat_of[FFFF] = 1
    return _build(words, 2, [0, 30, -20, 10], cat_of, [0, 1, 1], [0, 1, 1], {0: [(0, 0, 2000)], 1: [(1, 0, 1500)], 2: [(1, 1, 1800), (0, 1, 1700)]}, cat_len=cat_len, cat0=2)


CHAR_CLAIMS_SHORT = [(6, ("unknown", 1, 4)), (6, ("unknown", 3, 4)), (1, ("matches", 0, 2)), (4, ("matches", 0, 2)), (8, ("unknown", 1, 2)), (9, ("unknown", 0, 2)),
                     (0, ("reachable", True))]
CHAR_CLAIMS_FULL = [(6, ("unknown", 2, 3)), (6, ("no_unknown", 1)), (6, ("unknown", 3, 4)), (5, ("unknown", 0, 2)), (1, ("matches", 0, 2)), (0, ("reachable", True))]


def _parked_case():
    sents = [A * 10 + X, X * 62 + A * 10, A * 9, A * 8, X + A * 11 + X]
    claims = [(0, ("matches", 1, 9)), (0, ("matches", 2, 8)), (1, ("matches", 63, 9)), (1, ("matches", 64, 8)), (2, ("matches", 0, 9)), (2, ("matches", 1, 8)),
              (3, ("matches", 0, 8)), (4, ("matches", 3, 9)), (4, ("matches", 4, 8))]
    return Case("parked matches", parked_dict, sents, claims)


def _long_key_case():
    sents = [A * 256 + X, A * 257, A * 255]
    claims = [(0, ("matches", 0, 9)), (0, ("longest", 0, 256)), (0, ("matches", 1, 8)), (0, ("longest", 1, 255)), (1, ("matches", 1, 9)), (1, ("matches", 2, 8)),
              (1, ("longest", 2, 255)), (2, ("matches", 0, 8)), (2, ("longest", 0, 255))]
    return Case("keys of 255 and 256 characters", long_key_dict, sents, claims)


def catalogue() -> list:
    return [_parked_case(), _long_key_case(), Case("chunk pairing", chunk_dict, *chunk_sentences()), Case("unknown length cap", chunk_dict, *cap_sentences()),
            Case("sweep step", sweep_dict, *sweep_sentences()), Case("unreachable predecessor", quirk_dict, QUIRK_SENTENCES, QUIRK_CLAIMS),
            Case("characters, short category table", lambda: chars_dict(0x3100), CHAR_SENTENCES, CHAR_CLAIMS_SHORT),
            Case("characters, full category table", lambda: chars_dict(65536), CHAR_SENTENCES, CHAR_CLAIMS_FULL)]


# ---- withdrawal, for the user dictionary --------------------------------------------------------------------------------------------------------------------------------
# (name, make, sentence, entry, the positions that lose their unknown nodes, the positions that keep them only because their category invokes)
UserCase = namedtuple("UserCase", "name make sentence entries withdrawn kept_by_invoke")
KA3 = KA * 3


def twin_dict(invoke=(0, 0, 1)):
    """k_user_forward: withdrawal is decided by `cinfo[cat].flags & CAT_INVOKE`.  あ and か are of two categories that differ in their invoke bit alone
    (grouped, one unknown record of the same morph); no word holds either."""
    return _build([("ん", 0, 0, 100)], 2, [0, 5, 9, 2], {A: 1, KA: 2}, list(invoke), [1, 1, 1], {0: [(0, 0, 3000)], 1: [(1, 1, 3000)], 2: [(1, 1, 3000)]})


def user_cases() -> list:
    import userdict_cases as U

    dear = lambda key: (key, 1, 0, 30000, ("user", key))   # noqa: E731  (an entry no path takes by choice: where it is taken, the nodes around it were withdrawn)
    s, e = U.WITHDRAWAL_SENTENCE, U.WITHDRAWAL_ENTRY
    return [UserCase("withdrawal, H does not invoke", lambda: U.withdrawal_dict(0), s, [e, dear(e[0])], {1}, set()),
            UserCase("withdrawal, H invokes", lambda: U.withdrawal_dict(1), s, [e, dear(e[0])], set(), {1}),
            UserCase("two categories, the invoke bit alone differs", twin_dict, A * 3 + KA3, [dear(A * 2), dear(KA * 2)], {0, 1}, {3, 4})]


def user_decisions(lat, text: str, entries, invoke) -> tuple:
    """-> (the positions whose unknown nodes tests/userdict_ref.widen withdraws, the positions where an entry matches, no known word starts and the
    unknown nodes stay because the category invokes)."""
    import userdict_ref as R

    w = R.widen(lat, text, entries, invoke)
    withdrawn = {lat.nodes[i].char_pos for i in w.withdrawn}
    known_at = {n.char_pos for n in lat.nodes if int(n.class_) == 1}
    unknown_at = {n.char_pos for n in lat.nodes if int(n.class_) == 2}
    hit = {n.start for n in w.nodes[w.n_lattice:]}
    return withdrawn, {q for q in hit if q in unknown_at and q not in known_at and invoke[q]}
