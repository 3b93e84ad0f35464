"""The dictionaries and sentences the search / extended mode tests share (tests/test_mode_cpu.py, tests/test_gpu_mode.py): a dictionary of compounds
with their parts, words at the length thresholds, words around every edge of the kanji list, a dictionary whose unknown kanji runs are long, and
what tests/nbest_cases.py has of ties and crowded positions.  Imports without a device."""
import random

import numpy as np

from nbest_cases import ALPHABET, CROWDED_SENTENCE, FIXTURE_INPUTS, conn_get_of, crowded_dict, pydict_of, tie_dict, tie_sentence  # noqa: F401

MODES = ("normal", "search", "extended")
DEFAULTS = (2, 3000, 7, 1700)

KANJI_COMPOUND, KANJI_PARTS = "関西国際空港", ("関西", "国際", "空港")
KANA_COMPOUND, KANA_PARTS = "ソフトウェアエンジニア", ("ソフト", "ウェア", "エンジニア")   # 11 characters
# (word, its parts, whether search mode with the default penalties takes the parts): a word costs 1000, its parts 2500 together, so the parts win
# exactly where the word's penalty is above 1500 -- the first penalty of either rule is (no part is long enough for one)
THRESHOLD = [
    ("東京", ("東", "京"), False),                      # 2 kanji: at the kanji length
    ("大阪府", ("大", "阪府"), True),                   # 3 kanji: 3000
    ("名古屋市", ("名古", "屋市"), True),               # 4 kanji: 6000
    ("abcdefg", ("abc", "defg"), False),                # 7 others: at the other length
    ("hijklmno", ("hijk", "lmno"), True),               # 8 others: 1700
    ("pqrstuvwx", ("pqrs", "tuvwx"), True),             # 9 others: 3400
    ("漢字語ア", ("漢字", "語ア"), False),              # 3 kanji and a kana: not all kanji, and 4 is no length for the other rule
    ("高校1年生A組担任", ("高校1年", "生A組担任"), True),   # 9 mixed: the other rule, 3400
]
# every edge of the kanji list from both sides; X makes the word 山X川, all kanji iff X is: the parts 山 | X川 win exactly then
EDGE_CHARS = [0x3004, 0x3005, 0x3006, 0x3007, 0x33FF, 0x3400, 0x4DBF, 0x4DC0, 0x4DFF, 0x4E00, 0x9FFF, 0xA000, 0xF8FF, 0xF900, 0xFAFF, 0xFB00,
              0x1FFFF, 0x20000, 0x3FFFF, 0x40000]
FILLER = "ぬねの"   # no word holds them: runs of the default category, unknown words that extended mode cuts up


def is_kanji_case(cp: int) -> bool:
    """The list of include/kanpyo_gpu.h, "search mode", as the cases expect it (tests/mode_ref.py has its own copy)."""
    return cp in (0x3005, 0x3007) or 0x3400 <= cp <= 0x4DBF or 0x4E00 <= cp <= 0x9FFF or 0xF900 <= cp <= 0xFAFF or 0x20000 <= cp <= 0x3FFFF


def edge_word(cp: int) -> str:
    return "山" + chr(cp) + "川"


def _from_words(words: dict, kanji_group: int):
    """Dict.from_parts over {surface: cost}: categories DEFAULT (grouped), KANJI, KANA (katakana, grouped), none invoked beside a known word; two
    context ids with small non-negative connection costs."""
    from kanpyo_amd.dict import Dict

    cat = np.zeros(65536, dtype=np.uint8)
    for lo, hi in ((0x3005, 0x3005), (0x3007, 0x3007), (0x3400, 0x4DBF), (0x4E00, 0x9FFF), (0xF900, 0xFAFF)):
        cat[lo : hi + 1] = 1
    cat[0x30A1:0x30FB] = 2
    recs = sorted(words, key=lambda w: w.encode("utf-8"))
    morphs = [(i % 2, (i // 2) % 2, words[w]) for i, w in enumerate(recs)]
    return Dict.from_parts(recs, np.array(morphs, dtype=np.int64), 2, 2, [0, 7, 11, 3], ["DEFAULT", "KANJI", "KANA"], cat, np.array([0, 0, 0], dtype=np.uint8),
                           np.array([1, kanji_group, 1], dtype=np.uint8), {0: (1, 1), 1: (2, 1), 2: (3, 1)}, [(0, 0, 3000), (1, 1, 3000), (0, 1, 3000)])


def mode_words() -> dict:
    """{surface: cost} of mode_dict: the compounds, the threshold words and the edge words, each word at 1000 and its parts at 2500 together."""
    words = {}
    for whole, parts in [(KANJI_COMPOUND, KANJI_PARTS), (KANA_COMPOUND, KANA_PARTS)] + [(w, p) for w, p, _ in THRESHOLD]:
        words[whole] = 1000
        for k, part in enumerate(parts):
            words[part] = 2500 // len(parts) + (1 if k < 2500 % len(parts) else 0)
    words["山"] = 1250
    for cp in EDGE_CHARS:
        words[edge_word(cp)] = 1000
        words[chr(cp) + "川"] = 1250
    return words


def mode_dict():
    return _from_words(mode_words(), 0)


def surfaces_of(whole: str, parts, split: bool) -> list:
    return list(parts) if split else [whole]


def compound_sentences() -> list:
    """The two compounds alone, in a row, and beside unknown words."""
    return [KANJI_COMPOUND, KANA_COMPOUND, KANJI_COMPOUND + KANA_COMPOUND, FILLER + KANJI_COMPOUND + FILLER[:2] + KANA_COMPOUND + FILLER[:1],
            KANJI_PARTS[0] + KANJI_COMPOUND + KANJI_PARTS[2]]


def threshold_sentences() -> list:
    return [w for w, _, _ in THRESHOLD] + ["".join(w for w, _, _ in THRESHOLD[:3]) + FILLER + THRESHOLD[6][0]]


def edge_sentences() -> list:
    return [edge_word(cp) for cp in EDGE_CHARS]


_POOL = [KANJI_COMPOUND, KANA_COMPOUND, "関西", "空港", "東京", "大阪府", "ぬ", "ぬね", "ねのぬ", "エンジニア"]


def seeded_sentence(rng) -> str:
    """One to four pieces of the compound dictionary's: compounds, parts, threshold words and unknown runs."""
    return "".join(rng.choice(_POOL) for _ in range(rng.randint(1, 4)))


def seeded_sentences(n: int, seed: int = 2024) -> list:
    rng = random.Random(seed)
    return [seeded_sentence(rng) for _ in range(n)]


def wide_dict():
    """Two characters, every word of one or two of them with 40 records of different morphs: 80 nodes end at a position in the middle of a
    sentence, so a target's predecessors take the forward kernel's lanes more than one round (crowded_dict has at most a dozen per position)."""
    from nbest_cases import _dict

    rng = random.Random(65)
    recs, morphs = [], []
    for w in sorted(["あ", "い", "ああ", "あい", "いあ", "いい"], key=lambda x: x.encode()):
        for _ in range(40):
            recs.append(w)
            morphs.append((rng.randrange(3), rng.randrange(3), rng.choice([0, 100, 200])))
    return _dict(recs, morphs, 3, [rng.choice([-100, 0, 100]) for _ in range(9)], "あい", 0)


def long_dict():
    """Kanji as a GROUPED category and one short word: a run of kanji is one unknown node, up to the reference's 1024 characters (lattice.rs:55)."""
    return _from_words({"東京": 1000}, 1)


LONG_SENTENCES = ["漢" * 65, "字" * 1025, "東京" + "漢" * 65 + "ぬ"]


def tie_penalties(rng) -> tuple:
    """Lengths from {1, 2} and penalties from {0, 100}: the tie dictionaries' costs are multiples of 100, so ties survive them."""
    return (rng.choice([1, 2]), rng.choice([0, 100]), rng.choice([1, 2]), rng.choice([0, 100]))


def tie_mode_case(seed: int):
    """-> (Dict, sentence of 1 to 7 characters, penalties), seeded: the tie dictionaries of tests/nbest_cases.py."""
    rng = random.Random(seed * 104729 + 7)
    return tie_dict(seed), tie_sentence(rng), tie_penalties(rng)
