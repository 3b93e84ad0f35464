"""The synthetic IPADIC-shaped generator (kanpyo_amd/synth.py) that bench.py and the GPU tests draw their dictionaries and corpora from: its output is
pinned, so that a benchmark run measures the same inputs from one revision to the next."""
import hashlib

import numpy as np


def test_draw_is_generator_choice():
    """synth._draw over a precomputed CDF makes the draws Generator.choice(pool, size, p=p) makes, and leaves the random stream where choice leaves it."""
    from kanpyo_amd.synth import _cdf, _draw, _zipf_weights

    for n, s, sizes in ((83, 0.9, [1, 3, 2, 7]), (20871, 1.05, [2, np.int64(1), 5]), (1, 1.0, [4])):
        pool = np.arange(n) + 0x3041
        p = _zipf_weights(n, s)
        c = _cdf(p)
        a, b = np.random.default_rng(n), np.random.default_rng(n)
        for k in sizes * 50:
            assert np.array_equal(_draw(a, pool, c, k), b.choice(pool, size=k, p=p))
            assert a.integers(0, 1 << 30) == b.integers(0, 1 << 30)


def _digest(sd, n):
    from kanpyo_amd import synth

    h = hashlib.sha256("\n".join(sd.surfaces).encode())
    h.update(sd.dict.morph_dict)
    h.update("\n".join(synth.make_corpus(sd, n, 1, "cfg2")).encode())
    return h.hexdigest()[:16]


def test_small_dictionaries_and_corpora_are_pinned():
    from kanpyo_amd import synth

    assert _digest(synth.build_dict(6000, seed=3), 500) == "0f7157edc9eaed15"
    assert _digest(synth.build_dict(5000, seed=7, dense=True), 500) == "5bf598e027aa4df4"
