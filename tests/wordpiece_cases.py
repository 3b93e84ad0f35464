"""Lists and words CHOSEN AGAINST the WordPiece matcher (kgpu_wordpiece.hip: wordpiece_match over the `initial` and `cont` byte tables; on the host
wordpiece_split of kgpu_wordpiece_table.cpp), shared by tests/test_wordpiece_cpu.py (the host split) and tests/test_gpu_wordpiece_adversarial.py (the
device): colliding prefixes, the tables' longest entries, max_word_chars from both sides, random lists over a small alphabet, and a batch that sends
every wavefront round the grid-stride loop twice.

Input construction only, like table_keys.py and lines_ref.py's crafted records: NO EXPECTED VALUE COMES FROM HERE.  What a test expects is
wordpiece_ref's / encode_spans_ref's answer on the words or records built here; Case.split() is wordpiece_ref.split_with, computed once per case and
never changed.  Nothing at import time needs a device, and nothing here needs the library."""
import numpy as np

import lines_ref as R
import table_keys as T
import wordpiece_ref as WP

U = R.UNKNOWN
UNK = 0                      # the unk id of every case: the list's first entry
ALPHABET = ["a", "b", "c", "é", "あ", "い", "ス", "𠮷"]   # characters of 1, 1, 1, 2, 3, 3, 3 and 4 bytes
SENTENCE_RECORDS = (1, 63, 64, 65, 129)                    # below, at and above a window of 64 records; three windows


class Case:
    """A list with its prefix and limit, and the sentences (lists of words, bytes) to run through it."""

    def __init__(self, name, vocab, sentences, prefix=b"##", max_chars=100):
        self.name, self.prefix, self.max_chars = name, prefix, max_chars
        self.vocab = list(dict.fromkeys(vocab))   # (a prefix of no bytes, or two pairs with one piece, may name an entry twice: listed once)
        self.sentences = [list(s) for s in sentences]
        self._split = None

    def words(self):
        """The distinct words, in order of appearance."""
        return list(dict.fromkeys(w for s in self.sentences for w in s))

    def tables(self):
        return WP.tables(self.vocab, self.prefix)

    def split(self):
        """{word: its ids by the reference}, computed once."""
        if self._split is None:
            tabs = self.tables()
            self._split = {w: WP.split_with(tabs, w, self.max_chars, UNK) for w in self.words()}
        return self._split

    def adopt(self, split):
        """{word: ids} that a caller has from the reference already (encode_spans_ref over the case's records, whose ids it asserts to be wordpiece_ref's),
        for every distinct word, in place of computing the splits a second time."""
        if self._split is None:
            assert set(split) == set(self.words())
            self._split = dict(split)

    def id_of(self, entry):
        return self.vocab.index(entry)

    def outcomes(self):
        """By the reference alone -> {"empty", "whole", "split", "unk", "dead"}: the distinct words by what they give.  "dead" (a subset of "unk"): a word
        within the limit whose first piece exists -- some later start has no piece."""
        initial = self.tables()[0]
        out = {k: 0 for k in ("empty", "whole", "split", "unk", "dead")}
        for w, ids in self.split().items():
            if not ids:
                out["empty"] += 1
            elif len(ids) > 1:
                out["split"] += 1
            elif w in initial and ids == [initial[w]]:
                out["whole"] += 1
            else:
                assert ids == [UNK]
                out["unk"] += 1
                starts = WP.char_starts(w)
                ends = starts[1:] + [len(w)]
                out["dead"] += len(starts) <= self.max_chars and any(w[:e] in initial for e in ends)
        return out

    def __repr__(self):
        return f"Case({self.name})"


def records(sentences, shift=False):
    """Sentences of words -> lines_ref's (utf8, offsets, tokens, tok_offsets): every word an unknown-class record (ids 0 and 1 in turn: without a row, and
    with the first unknown row, whose word is the surface) over the sentence's words back to back; start / end are the characters in front of the
    record's first byte and of the byte behind its last.
    shift: every record starts ONE BYTE LATER and is as long (one byte shorter at the sentence's end): behind a multi-byte character's first byte the word
    then begins with 10xxxxxx bytes, and it may end inside a character."""
    texts, recs, chars = [], [], []
    for words in sentences:
        text = b"".join(words)
        lead = np.concatenate([[0], np.cumsum((np.frombuffer(text, dtype=np.uint8) & 0xC0) != 0x80)]).tolist()
        at, r = 0, []
        for j, w in enumerate(words):
            pos, n = at, len(w)
            if shift and n:
                pos, n = at + 1, min(n, len(text) - at - 1)
            r.append((j % 2, U, pos, n))
            chars.append((lead[pos], lead[pos + n]))
            at += len(w)
        texts.append(text)
        recs.append(r)
    case = R.pack(texts, recs)
    if chars:
        case[2]["start"], case[2]["end"] = [c[0] for c in chars], [c[1] for c in chars]
    return case


def record_words(case):
    """The byte strings the records of a packed case name, per sentence (what `shift` made of the words)."""
    utf8, offsets, tokens, toff = case
    raw = utf8.tobytes()
    out = []
    for s in range(len(offsets) - 1):
        base = int(offsets[s])
        out.append([raw[base + int(t["position"]): base + int(t["position"]) + int(t["byte_len"])] for t in tokens[int(toff[s]): int(toff[s + 1])]])
    return out


def spread(words):
    """All the words in one sentence (neighbouring lanes of one window), the same backwards, then every word in a sentence of its own."""
    return [list(words), list(words)[::-1]] + [[w] for w in words]


def by_length(words, lengths=SENTENCE_RECORDS):
    """The words in order over sentences of 1, 63, 64, 65, 129, 1, 63, ... records."""
    out, at, k = [], 0, 0
    while at < len(words):
        out.append(words[at: at + lengths[k % len(lengths)]])
        at += lengths[k % len(lengths)]
        k += 1
    return out


# ---- A. colliding prefixes ----------------------------------------------------------------------------------------------------------------------------
BASE = [b"[UNK]", b"X", b"##c"]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def proper_prefix(a, k):
    """A proper prefix of a, one byte long at least; k varies its length from pair to pair."""
    return a[: 1 + k % (len(a) - 1)]


def twin_cases():
    """Equal length, only the twin listed: ##b and ##s (s a proper prefix of a); the words X a, X a c, X a b (and X b, X s c, which split, and X a !, which
    never does).  At prefix
    length |a| the probe meets a slot whose tag carries a's hash and whose entry has a's length and other bytes.  "dead": what follows s in a is not
    listed -- the three words are [UNK]; "split": it is.  -> [(case, [(a, b, s)])]"""
    def make():
        same = T.wordpiece_pairs()[0]
        out = []
        for variant in ("dead", "split"):
            vocab, words, trios = list(BASE), [], []
            for k, (a, b) in enumerate(same):
                s = proper_prefix(a, k)
                vocab += [b"##" + b, b"##" + s] + ([b"##" + a[len(s):]] if variant == "split" else [])
                words += [b"X" + a, b"X" + a + b"c", b"X" + a + b, b"X" + b, b"X" + s + b"c", b"X" + a + b"!"]
                trios.append((a, b, s))
            out.append((Case("twin-" + variant, vocab, spread(words)), trios))
        return out
    return _cached("twin", make)


def both_listed_case():
    """##a and ##b listed: X a b and X b a side by side (one hash, one home slot, two entries), and X a ! -- a dead end behind a colliding piece."""
    def make():
        same = T.wordpiece_pairs()[0]
        vocab, words = list(BASE), []
        for a, b in same:
            vocab += [b"##" + a, b"##" + b]
            words += [b"X" + a + b, b"X" + b + a, b"X" + a + b"!", b"X" + b + b"c"]
        return Case("both-listed", vocab, spread(words)), same
    return _cached("both", make)


def cross_length_cases():
    """|a| = 8, |b| = 7, one hash (the random pairs, and the nested ones whose b IS a's first seven bytes).  "long": ##a alone is listed and X b c is asked
    -- the 7-byte prefix carries the hash of the 8-byte entry; "short": ##b alone and X a c.  "+pieces": the asked key's first three bytes and its rest are
    listed too, so the word splits around the probe that must miss.  -> [(case, [(listed key, asked key)])]"""
    def make():
        _, cross, nested = T.wordpiece_pairs()
        out = []
        for listed in ("long", "short"):
            for pieces in (False, True):
                vocab, words, asked = list(BASE), [], []
                for a, b in cross + nested:
                    have, ask = (a, b) if listed == "long" else (b, a)
                    vocab.append(b"##" + have)
                    if pieces:
                        vocab += [b"##" + ask[:3], b"##" + ask[3:]]
                    words += [b"X" + ask + b"c", b"X" + ask, b"X" + have, b"X" + have + b"c", b"X" + have + b"!"]
                    asked.append((have, ask))
                out.append((Case(f"cross-{listed}{'+pieces' if pieces else ''}", vocab, spread(words)), asked))
        return out
    return _cached("cross", make)


def both_tables_cases():
    """The same bytes k in both tables with different ids (k and ##k listed), for "##" and for the prefix of no bytes (ONE shared table, where ##k is a
    plain entry): the words k, X k, k k, ##k, and X k ! (a dead end)."""
    def make():
        same, cross, _ = T.wordpiece_pairs()
        keys = [same[0][0], same[0][1], cross[0][0], cross[0][1], "é".encode(), "あい".encode(), b"ab"]
        out = []
        for prefix in (b"##", b""):
            vocab, words = list(BASE), []
            for k in keys:
                vocab += [k, b"##" + k]
                words += [k, b"X" + k, k + k, b"##" + k, b"X" + k + b"!", k + b"c"]
            out.append((Case("both-tables" + ("" if prefix else "-shared"), vocab, spread(words), prefix=prefix), keys))
        return out
    return _cached("tables", make)


def chain_cases():
    """Eight ## entries whose home is slot 15 of the 16-slot continuation table: the chain wraps round the table's end.  X + every chain key, every absent
    key of that home (its probe walks the whole chain to the free slot) and the keys whose home the chain covers, four times over in ONE sentence of 76
    records; and 256 sentences holding them once, rotated.  -> (one-sentence case, rotated case, (chain, absent, covered))"""
    def make():
        chain, absent, covered = T.chain(16, 15, 8, byte_range=T.PRINTABLE)
        vocab = [b"[UNK]", b"X"] + [b"##" + k for k in chain]   # (no ##c: a ninth continuation entry would double the table)
        words = [b"X" + k for trio in zip(chain, (absent * 2)[:8], covered + covered[:1]) for k in trio]
        words = list(dict.fromkeys(words + [b"X" + k for k in absent + covered]))
        assert len(words) == 8 + 4 + 7
        one = Case("chain-one-sentence", vocab, [words * 4])
        rotated = Case("chain-rotated", vocab, [words[s % len(words):] + words[: s % len(words)] for s in range(256)])
        return one, rotated, (chain, absent, covered)
    return _cached("chain", make)


# ---- B. the tables' longest entries ----------------------------------------------------------------------------------------------------------------------
LONG24 = b"abcdefghijklmnopqrstuvwx"


def longest_entry_cases():
    """-> [case]: "initial-24" -- the longest initial entry has 24 bytes, the continuation entries 3 at the most; "cont-24" -- the reverse (the 24-byte
    continuation entry is, behind its prefix, a 26-byte initial entry); "inside-@" / "inside-##" -- the longest entry is abcd (4 bytes; with "##" the
    5-byte ##あ) and the bound of abcあ's first start falls inside あ, where no piece may end; "no-cont" -- no entry carries the prefix."""
    def make():
        assert len(LONG24) == 24
        a = Case("initial-24", [b"?", b"X", b"##c", b"##cd", b"##yz!", b"abc", LONG24],
                 spread([LONG24, LONG24 + b"c", LONG24 + b"cd", LONG24 + b"yz!", LONG24[:23], LONG24 + b"x", b"abc" + b"yz!", b"Xcdc", b"abcd"]))
        b = Case("cont-24", [b"?", b"X", b"ab", b"##c", b"##" + LONG24],
                 spread([b"X" + LONG24, b"X" + LONG24 + b"c", b"##" + LONG24, b"X" + LONG24[:23], b"ab" + LONG24 + LONG24, b"X" + LONG24[1:], b"Xc", b"abc"]))
        ai = "あ".encode()
        inside = [Case("inside-" + p.decode(), [b"?", b"abcd", b"abc", p + ai, b"X", p + b"bcd"],
                       spread([b"abc" + ai, b"abcd" + ai, b"ab" + ai, b"abcd" + ai + "い".encode(), b"Xbcd" + ai, b"Xbc" + ai, b"abcd", ai + b"abc"]), prefix=p)
                  for p in (b"@", b"##")]
        none = Case("no-cont", [b"?", b"a", b"ab", b"abc", ai, b"#", b"##"], spread([b"abc", b"abcd", b"aba", b"a", ai + b"a", ai, b"##", b"##a", b"#a", b"ab" + ai]))
        return [a, b] + inside + [none]
    return _cached("longest", make)


# ---- C. max_word_chars from both sides ----------------------------------------------------------------------------------------------------------------------
CHARS = [c.encode() for c in ("a", "é", "あ", "𠮷")]   # 1, 2, 3 and 4 bytes
LIMITS = (1, 2, 100, 1024)


def limit_case(limit):
    """Every character listed alone and behind the prefix; words of limit - 1, limit and limit + 1 characters of one kind, and of the four kinds in turn.
    -> (case, {word: its characters})"""
    def make():
        vocab = [b"[UNK]"] + CHARS + [b"##" + c for c in CHARS]
        count = {}
        for n in (limit - 1, limit, limit + 1):
            for c in CHARS:
                count[c * n] = n
            count[b"".join(CHARS[k % 4] for k in range(n))] = n
        words = list(count)
        return Case(f"limit-{limit}", vocab, [words, words[::-1]], max_chars=limit), count
    return _cached(("limit", limit), make)


def full_window_case():
    """ONE sentence of 64 records that all name one word of 1024 four-byte characters (4096 bytes, laid down once): 64 x 1024 ids from one window."""
    def make():
        vocab = [b"[UNK]"] + CHARS + [b"##" + c for c in CHARS]
        return Case("full-window", vocab, [[CHARS[3] * 1024]], max_chars=1024)
    return _cached("window", make)


def full_window_records(case):
    word, = case.words()
    recs = R.pack([word], [[(j % 2, U, 0, len(word)) for j in range(64)]])
    recs[2]["end"] = 1024
    return recs


# ---- D. random lists over a small alphabet ---------------------------------------------------------------------------------------------------------------------
PREFIXES = (b"##", b"@", b"", "##あい".encode())   # 2, 1, 0 and 8 bytes (WORDPIECE_MAX_PREFIX)
RANDOM_LIMITS = (100, 6)
CONDITIONS = {"split": 100, "unk": 100, "dead": 50, "whole": 5}


def _random_case(prefix, limit, seed):
    rng = np.random.default_rng(seed)
    word = lambda n: "".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=n)).encode()   # noqa: E731
    # one character is missing as a single-character entry from each table (with every letter listed, the prefix of no bytes would leave no [UNK] at all)
    gone = [ALPHABET[i].encode() for i in rng.choice(len(ALPHABET), 2, replace=False)]
    vocab = [b"[UNK]"]
    for _ in range(150):
        w = word(int(rng.integers(1, 4)))
        behind = bool(rng.integers(0, 2))
        if w == gone[behind] or (not prefix and w in gone):
            continue
        vocab.append(prefix + w if behind else w)
    words = [word(int(rng.integers(1, 10))) for _ in range(1500)]
    return Case(f"random-{prefix.decode()!r}-{limit}-seed{seed}", vocab, by_length(words), prefix=prefix, max_chars=limit)


def meets(case):
    got = case.outcomes()
    return all(got[k] >= n for k, n in CONDITIONS.items())


def random_case(prefix, limit):
    """About 150 entries of 1 to 3 characters, half behind the prefix; 1500 words of 1 to 9 characters over sentences of 1, 63, 64, 65 and 129 records.  A draw
    that misses CONDITIONS (by the reference) is drawn again with the next seed -- never dropped."""
    def make():
        for seed in range(1000 * PREFIXES.index(prefix) + limit, 1000 * PREFIXES.index(prefix) + limit + 20):
            case = _random_case(prefix, limit, seed)
            if meets(case):
                return case
        raise ValueError(f"prefix {prefix!r}, limit {limit}: no seed of 20 meets {CONDITIONS}")
    return _cached(("random", prefix, limit), make)


# ---- E. second trips of the grid-stride loops -----------------------------------------------------------------------------------------------------------------
GRID_BLOCKS = 8192             # launch_render's cap (kgpu_records_dev.h)
SECOND_TRIP_N = 32768 + 300
LONG_AT = (0, 32768, SECOND_TRIP_N - 1)


def render_wpb():
    """RENDER_WPB as kgpu_records_dev.h states it."""
    import os
    import re

    from conftest import ROOT

    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_records_dev.h"), encoding="utf-8") as f:
        return int(re.search(r"constexpr uint32_t RENDER_WPB = (\d+);", f.read()).group(1))


def second_trip_list():
    """[UNK], every byte that starts a character alone and behind "##", the pieces of the fixture dictionary's first key and its second key whole."""
    singles = [bytes([c]) for c in list(range(1, 0x80)) + list(range(0xC0, 0x100))]
    return [b"[UNK]"] + singles + [b"##" + c for c in singles] + [w.encode() for w in ("テ", "##ス", "##ト", "辞書")]


def second_trip_records(n_known, n_unk):
    """lines_ref.many_case with SECOND_TRIP_N sentences of 0 to 3 short records over random bytes; sentences 0, 32 768 and the last have 200."""
    return _cached(("trips", n_known, n_unk), lambda: R.many_case(np.random.default_rng(41), SECOND_TRIP_N, n_known, n_unk, long_at=LONG_AT))


# ---- what every case claims to be, asserted by the reference alone (both test modules call these first) ---------------------------------------------------------
def _both_outcomes(case):
    got = case.outcomes()
    assert got["split"] > 0 and got["unk"] > 0, (case, got)


def claim_twin(case, trios):
    import encode_ref as E

    sp = case.split()
    for a, b, s in trios:
        assert E.key_hash(a) == E.key_hash(b) and a != b and len(a) == len(b) and a.startswith(s) and 0 < len(s) < len(a)
        ib, is_, x = case.id_of(b"##" + b), case.id_of(b"##" + s), case.id_of(b"X")
        assert b"##" + a not in case.vocab
        if case.name == "twin-dead":
            assert sp[b"X" + a] == sp[b"X" + a + b"c"] == sp[b"X" + a + b] == [UNK], "X ##s, then a dead end: the whole word is [UNK]"
        else:
            rest = case.id_of(b"##" + a[len(s):])
            assert sp[b"X" + a] == [x, is_, rest] and sp[b"X" + a + b"c"] == [x, is_, rest, case.id_of(b"##c")] and sp[b"X" + a + b] == [x, is_, rest, ib]
        assert ib not in sp[b"X" + a] + sp[b"X" + a + b"c"], "no expected id is b's where a's bytes stand"
        assert sp[b"X" + b] == [x, ib]
    _both_outcomes(case)


def claim_both_listed(case, pairs):
    import encode_ref as E

    sp = case.split()
    x = case.id_of(b"X")
    for a, b in pairs:
        ia, ib = case.id_of(b"##" + a), case.id_of(b"##" + b)
        assert E.key_hash(a) == E.key_hash(b) and a != b and ia != ib
        assert sp[b"X" + a + b] == [x, ia, ib] and sp[b"X" + b + a] == [x, ib, ia] and sp[b"X" + a + b"!"] == [UNK], "each piece has its own id"
    first = case.sentences[0]
    assert all(first[4 * k: 4 * k + 2] == [b"X" + a + b, b"X" + b + a] for k, (a, b) in enumerate(pairs)), "the two words are neighbours in one window"
    assert [b"X" + pairs[0][0] + pairs[0][1]] in case.sentences and [b"X" + pairs[0][1] + pairs[0][0]] in case.sentences, "... and alone in sentences of their own"
    _both_outcomes(case)


def claim_cross(case, asked):
    import encode_ref as E

    sp = case.split()
    x = case.id_of(b"X")
    for have, ask in asked:
        assert E.key_hash(have) == E.key_hash(ask) and {len(have), len(ask)} == {7, 8}
        ih = case.id_of(b"##" + have)
        assert b"##" + ask not in case.vocab
        got = sp[b"X" + ask + b"c"]
        if ask.startswith(have):   # (nested, the short key listed: the listed key IS a piece of the asked one)
            assert got == [UNK] or got[:2] == [x, ih]
        else:
            assert ih not in got and ih not in sp[b"X" + ask], "never the listed key's id"
        assert sp[b"X" + have] == [x, ih] and sp[b"X" + have + b"c"] == [x, ih, case.id_of(b"##c")]
        if "+pieces" in case.name and not ask.startswith(have):
            assert got == [x, case.id_of(b"##" + ask[:3]), case.id_of(b"##" + ask[3:]), case.id_of(b"##c")], "split around the probe that must miss"
        elif "+pieces" not in case.name and not ask.startswith(have):
            assert got == [UNK]
    assert any(h.startswith(a) or a.startswith(h) for h, a in asked), "a pair whose short key is the long key's first bytes"
    _both_outcomes(case)


def claim_both_tables(case, keys):
    sp = case.split()
    x = case.id_of(b"X")
    for k in keys:
        plain, behind = case.id_of(k), case.id_of(b"##" + k)
        assert plain != behind
        if case.prefix:
            assert sp[k] == [plain] and sp[b"X" + k] == [x, behind] and sp[k + k] == [plain, behind] and sp[b"##" + k] == [behind], "the right table's id at the right start"
        else:
            assert sp[k] == [plain] and sp[b"X" + k] == [x, plain] and sp[k + k] == [plain, plain] and sp[b"##" + k] == [behind], "one shared table"
        assert sp[b"X" + k + b"!"] == [UNK]
    _both_outcomes(case)


def claim_chain(one, rotated, keys):
    import encode_ref as E

    chain, absent, covered = keys
    assert all(E.key_hash(k) & 15 == 15 for k in chain + absent) and [E.key_hash(k) & 15 for k in covered] == list(range(7))
    assert len(one.sentences) == 1 and len(one.sentences[0]) > 64 and len(rotated.sentences) == 256 and rotated.sentences[1] == rotated.sentences[0][1:] + rotated.sentences[0][:1]
    assert sum(1 for w in one.vocab if w.startswith(b"##")) == 8, "eight continuation entries: a table of 16 slots"
    for case in (one, rotated):
        sp = case.split()
        x = case.id_of(b"X")
        assert all(sp[b"X" + k] == [x, case.id_of(b"##" + k)] for k in chain) and all(sp[b"X" + k] == [UNK] for k in absent + covered)
        _both_outcomes(case)


def claim_longest(case):
    sp = case.split()
    ids = case.id_of
    if case.name == "initial-24":
        assert max(len(w) for w in case.vocab) == 24 and max(len(w) - 2 for w in case.vocab if w.startswith(b"##")) == 3
        assert sp[LONG24] == [ids(LONG24)] and sp[LONG24 + b"c"] == [ids(LONG24), ids(b"##c")] and sp[LONG24 + b"yz!"] == [ids(LONG24), ids(b"##yz!")]
        assert sp[LONG24[:23]] == [UNK] and sp[LONG24 + b"x"] == [UNK] and sp[b"abcyz!"] == [ids(b"abc"), ids(b"##yz!")]
    elif case.name == "cont-24":
        long = b"##" + LONG24
        assert max(len(w) for w in case.vocab) == 26 and max(len(w) - 2 for w in case.vocab if w.startswith(b"##")) == 24
        assert sp[b"X" + LONG24] == [ids(b"X"), ids(long)] and sp[b"X" + LONG24 + b"c"] == [ids(b"X"), ids(long), ids(b"##c")] and sp[long] == [ids(long)]
        assert sp[b"ab" + LONG24 + LONG24] == [ids(b"ab"), ids(long), ids(long)] and sp[b"X" + LONG24[:23]] == [UNK]
    elif case.name.startswith("inside-"):
        p, ai = case.prefix, "あ".encode()
        assert max(len(w) for w in case.vocab) == (4 if p == b"@" else 5), "the bound of the first start falls inside あ"
        assert sp[b"abc" + ai] == [ids(b"abc"), ids(p + ai)] and sp[b"abcd" + ai] == [ids(b"abcd"), ids(p + ai)] and sp[b"ab" + ai] == [UNK]
        assert sp[b"Xbcd" + ai] == [ids(b"X"), ids(p + b"bcd"), ids(p + ai)] and sp[b"Xbc" + ai] == [UNK]
    else:
        assert case.name == "no-cont" and case.tables()[1] == {}, "no entry carries the prefix"
        listed = set(case.vocab)
        assert all(sp[w] == ([ids(w)] if w in listed else [UNK]) for w in case.words()), "a word listed whole is itself, every other one [UNK]"
        assert case.outcomes()["whole"] >= 4 and case.outcomes()["dead"] >= 4 and case.outcomes()["split"] == 0
        return
    _both_outcomes(case)


def claim_limit(case, count, limit):
    sp = case.split()
    assert case.max_chars == limit and set(count.values()) == {limit - 1, limit, limit + 1}
    for w, n in count.items():
        assert len(WP.char_starts(w)) == n
        assert len(sp[w]) == (n if n <= limit else 1), "below and at the limit as many pieces as characters; one above it, one [UNK]"
        assert (sp[w] == [UNK]) == (n > limit)
    assert max(len(w) for w in count) == 4 * (limit + 1)


def claim_full_window(case):
    word, = case.words()
    assert len(word) == 4096 and len(case.split()[word]) == 1024 and UNK not in case.split()[word]


def claim_random(case):
    got = case.outcomes()
    assert all(got[k] >= n for k, n in CONDITIONS.items()), (case, got)
    assert sorted({len(s) for s in case.sentences[:5]}) == sorted(SENTENCE_RECORDS) and sum(len(s) for s in case.sentences) == 1500
    singles = {c.encode() for c in ALPHABET}
    initial, cont = case.tables()
    assert singles - set(initial) and singles - set(cont), "a character is missing as a single-character entry from each table"
