"""The dictionaries and constants the lattice-probability tests share (tests/test_prob_cpu.py, tests/test_gpu_prob.py): the tie dictionaries and fixture
inputs of the N-best tests, and a wide dictionary whose middle positions have more than 128 nodes ending and more than 128 starting there -- three
rounds of 64 in the forward and in the backward kernel.  Imports without a device."""
import random

from nbest_cases import FIXTURE_INPUTS, _dict, tie_dict, tie_sentence  # noqa: F401

THETAS = (0.75 / 800, 0.01, 1e-6, 1.0)   # the default; sharper; nearly uniform; so sharp that most terms of a sum underflow to 0
WIDE_SENTENCES = ("あ" * 6, "あ" * 2)


def wide_dict():
    """One character; 70 records each for the words of one and of two of it, morphs differing (costs 0 .. 300, three context ids)."""
    rng = random.Random(70)
    recs, morphs = [], []
    for w in ("あ", "ああ"):
        for _ in range(70):
            recs.append(w)
            morphs.append((rng.randrange(3), rng.randrange(3), rng.choice([0, 100, 200, 300])))
    return _dict(recs, morphs, 3, [rng.choice([-100, 0, 100]) for _ in range(9)], "あ", 0)


def widths(lat) -> tuple:
    """-> (the most nodes that end at one position, the most that start at one), read off a lattice (EOS and BOS left out)."""
    ends, starts = {}, {}
    for n in lat.nodes[1:-1]:
        ends[n.end_char] = ends.get(n.end_char, 0) + 1
        starts[n.char_pos] = starts.get(n.char_pos, 0) + 1
    return max(ends.values(), default=0), max(starts.values(), default=0)


def tie_case(seed: int):
    """-> (Dict, sentence of 1 to 7 characters), seeded (nbest_cases.tie_case without its k)."""
    rng = random.Random(seed * 7919 + 1)
    return tie_dict(seed), tie_sentence(rng)
