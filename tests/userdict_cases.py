"""The dictionaries, sentences and entries the user dictionary tests share (tests/test_userdict_cpu.py, tests/test_gpu_userdict.py): the tie
dictionaries of tests/nbest_cases.py with entries cut from the sentence (ties between user nodes, and between a user node and a lattice node, are
certain), dictionaries with wide-ranging costs whose entries can also be merged into the keyword list, the crafted withdrawal cases, and keys that are
the hash table's worst cases (tests/table_keys.py).  An entry is (surface, left_id, right_id, cost, features).  Imports without a device."""
import random

import numpy as np

import table_keys as TK
from mode_cases import DEFAULTS, MODES, tie_penalties  # noqa: F401
from nbest_cases import ALPHABET, _dict, tie_dict, tie_sentence

NEVER = ("ん", "あいうえあいうえ", "z")   # keys no sentence of the alphabet holds: another character, longer than any sentence, ASCII


def entries_from(rng, sentence: str, n: int, costs, nctx: int = 3, max_len: int = 3) -> list:
    """n entries whose keys are substrings of the sentence (a key may come more than once), then the keys that never match."""
    out = []
    for _ in range(n if sentence else 0):
        a = rng.randrange(len(sentence))
        key = sentence[a : a + rng.randint(1, max_len)]
        out.append((key, rng.randrange(nctx), rng.randrange(nctx), rng.choice(costs) if isinstance(costs, (list, tuple)) else costs(rng), ("user", key)))
    for key in NEVER[: rng.randint(0, 3)]:
        out.append((key, rng.randrange(nctx), rng.randrange(nctx), 0, ("never", key)))
    rng.shuffle(out)
    return out


def tie_user_case(seed: int):
    """-> (Dict, sentence of 1 to 7 characters, entries, penalties), seeded: a tie dictionary, 0 to 6 entries with costs from {0, 100} (its words')."""
    rng = random.Random(seed * 15485863 + 11)
    s = tie_sentence(rng)
    return tie_dict(seed), s, entries_from(rng, s, rng.randint(0, 6), [0, 100]), tie_penalties(rng)


def _wide_parts(seed: int):
    """The parts of a dictionary over the alphabet with costs from a wide range (a unique best path is likely), and a sentence with entries."""
    rng = random.Random(seed * 32452843 + 5)
    words = set()
    want = rng.randint(6, 20)
    while len(words) < want:
        words.add("".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 3))))
    recs = sorted(words, key=lambda x: x.encode())
    morphs = [(rng.randrange(3), rng.randrange(3), rng.randint(-2000, 6000)) for _ in recs]
    conn = [rng.randint(-700, 700) for _ in range(9)]
    s = "".join(rng.choice(ALPHABET) for _ in range(rng.randint(2, 8)))
    entries = entries_from(rng, s, rng.randint(1, 5), lambda r: r.randint(-2000, 6000))
    return recs, morphs, conn, rng.randrange(2), s, entries


def wide_user_case(seed: int):
    """-> (Dict, the Dict with the entries among its keywords, sentence, entries): every character has an unknown category, so EOS is always reachable."""
    recs, morphs, conn, group, s, entries = _wide_parts(seed)
    merged = sorted(list(zip(recs, morphs)) + [(e[0], (e[1], e[2], e[3])) for e in entries], key=lambda rm: rm[0].encode())
    alphabet = ALPHABET + "んz"   # (the never-matching keys' characters are of the alphabet's category in BOTH dictionaries: the sentence has none of them)
    return (_dict(recs, morphs, 3, conn, alphabet, group), _dict([r for r, _ in merged], [m for _, m in merged], 3, conn, alphabet, group), s, entries)


# ---- withdrawal, crafted --------------------------------------------------------------------------------------------------------------------------------------
def withdrawal_dict(invoke_h: int):
    """Known words い and うえ; the alphabet's category H is grouped and has an unknown word; invoke_h: whether H invokes unknown words beside a known one."""
    from kanpyo_amd.dict import Dict

    cat = np.zeros(65536, dtype=np.uint8)
    for ch in ALPHABET:
        cat[ord(ch)] = 1
    recs = sorted(["い", "うえ"], key=lambda x: x.encode())
    return Dict.from_parts(recs, np.array([(0, 0, 500), (1, 1, 500)], dtype=np.int64), 2, 2, [0, 5, 9, 2], ["DEFAULT", "H"], cat, np.array([0, invoke_h], dtype=np.uint8),
                           np.array([1, 0], dtype=np.uint8), {0: (1, 1), 1: (2, 1)}, [(0, 0, 3000), (1, 1, 3000)])


WITHDRAWAL_SENTENCE = "ああいうえ"
WITHDRAWAL_ENTRY = ("あい", 1, 0, 100, ("user", "あい"))   # matches at 1, inside the run of H: no known word starts there


# ---- the table's worst cases ------------------------------------------------------------------------------------------------------------------------------------
def table_worst_keys() -> dict:
    """ASCII keys (one-byte characters: valid UTF-8, every byte a character) built with tests/table_keys.py:
    colliding   pairs of different keys with ONE full hash (equal length, and of two lengths): a tag's hash selects both, the bytes must decide
    crowded     24 keys of one home slot of the 64-slot table they fill with the 8 others: one chain that wraps around the table's end
    prefixes    keys that share every character but the last"""
    same = TK.colliding_pairs(5, 3, seed=71, byte_range=TK.PRINTABLE) + TK.colliding_pairs(8, 2, seed=72, byte_range=TK.PRINTABLE)
    cross = TK.cross_length_pairs(5, 6, 2, seed=73, byte_range=TK.PRINTABLE)
    crowded = TK.keys_with_home(64, 63, 24, 6, seed=74, byte_range=TK.PRINTABLE)
    prefixes = ["abcdefg" + c for c in "hijklmnop"] + ["abcdefg"]
    return {"colliding": [k.decode() for p in same + cross for k in p], "crowded": [k.decode() for k in crowded], "prefixes": prefixes}


def ascii_dict():
    """No known word at all over printable ASCII: category 0 (grouped, invoking nothing) gives one unknown word per run, which an entry withdraws."""
    from kanpyo_amd.dict import Dict

    cat = np.zeros(65536, dtype=np.uint8)
    return Dict.from_parts(["~~~~"], np.array([(0, 0, 10)], dtype=np.int64), 2, 2, [0, 3, 4, 1], ["DEFAULT"], cat, np.array([0], dtype=np.uint8), np.array([1], dtype=np.uint8),
                           {0: (1, 1)}, [(0, 0, 5000)])


def sentences_over(keys, rng, n: int) -> list:
    """n sentences of two to four keys in a row, with a character no key holds between some of them."""
    return ["".join(rng.choice(keys) + rng.choice(["", " "]) for _ in range(rng.randint(2, 4))) for _ in range(n)]
