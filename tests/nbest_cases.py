"""The dictionaries and sentences the N-best tests share (tests/test_nbest_cpu.py, tests/test_gpu_nbest.py): small tie-heavy dictionaries, a crowded one
whose targets have more than 64 candidates, and what both tests read off a lattice.  Imports without a device."""
import random

import numpy as np

ALPHABET = "あいうえ"
TIE_KS = (1, 2, 3, 5, 8, 64)
FIXTURE_INPUTS = ["", "テスト", "テ", "テあ", "あいうえお", "辞書形態素"]


def _dict(recs, morphs, nctx, conn, alphabet, group):
    """Dict.from_parts over sorted records: the alphabet is one category (never invoked beside a known word), everything else the default one."""
    from kanpyo_amd.dict import Dict

    cat = np.zeros(65536, dtype=np.uint8)
    for ch in alphabet:
        cat[ord(ch)] = 1
    return Dict.from_parts(recs, np.array(morphs, dtype=np.int64), nctx, nctx, conn, ["DEFAULT", "H"], cat, np.array([0, 0], dtype=np.uint8),
                           np.array([1, group], dtype=np.uint8), {0: (1, 1), 1: (2, 1)}, [(0, 0, 100), (1 % nctx, 1 % nctx, 100)])


def tie_dict(seed: int):
    """20 to 60 surfaces of 1 to 3 characters over an alphabet of 4, each with 1 to 3 records of EQUAL morphs (exact ties are certain), morph costs
    from {0, 100}, matrix entries from {-100, 0, 100} over 3 context ids."""
    rng = random.Random(seed)
    words = set()
    want = rng.randint(20, 60)
    while len(words) < want:
        words.add("".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 3))))
    recs, morphs = [], []
    for w in sorted(words, key=lambda x: x.encode()):
        m = (rng.randrange(3), rng.randrange(3), rng.choice([0, 100]))
        for _ in range(rng.choice([1, 1, 2, 3])):
            recs.append(w)
            morphs.append(m)
    conn = [rng.choice([-100, 0, 100]) for _ in range(9)]
    return _dict(recs, morphs, 3, conn, ALPHABET, rng.randrange(2))


def tie_sentence(rng) -> str:
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 7)))


def tie_case(seed: int):
    """-> (Dict, sentence of 1 to 7 characters, k from TIE_KS), seeded."""
    rng = random.Random(seed * 7919 + 1)
    return tie_dict(seed), tie_sentence(rng), rng.choice(TIE_KS)


def crowded_dict():
    """Two characters, every word of one to three of them with four records of different morphs: a position in the middle of a sentence has dozens of
    predecessors, each with a full list."""
    rng = random.Random(64)
    recs, morphs = [], []
    words = sorted({a + b + c for a in ["", "あ", "い"] for b in ["", "あ", "い"] for c in ["あ", "い"]}, key=lambda x: x.encode())
    for w in words:
        for _ in range(4):
            recs.append(w)
            morphs.append((rng.randrange(3), rng.randrange(3), rng.choice([0, 100, 200])))
    return _dict(recs, morphs, 3, [rng.choice([-100, 0, 100]) for _ in range(9)], "あい", 0)


CROWDED_SENTENCE = "あいあいいあああいあ"


def conn_get_of(d):
    """ConnectionTable::get of a Dict, from its own blob (connection.rs:12-14, 44-51)."""
    import struct

    rows, _ = struct.unpack_from("<QQ", bytes(d.connection_dict), 0)
    data = np.frombuffer(bytes(d.connection_dict), dtype="<i2", offset=16)
    return lambda r, l: int(data[rows * l + r])


def pydict_of(d):
    from oracle import pyref

    return pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)


def max_candidates(lat, k: int) -> tuple:
    """-> (the most predecessors a node has, the most candidates a target has with n_best = k): a predecessor offers min(k, its paths from BOS)."""
    paths = [0] * len(lat.nodes)
    paths[0] = 1
    widest, most = 0, 0
    for t in range(1, len(lat.nodes)):
        pred = lat.edges[lat.nodes[t].char_pos]
        paths[t] = sum(paths[j] for j in pred)
        widest, most = max(widest, len(pred)), max(most, sum(min(k, paths[j]) for j in pred))
    return widest, most
