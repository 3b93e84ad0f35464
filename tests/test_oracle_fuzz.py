"""Differential fuzz of the two CPU restatements (oracle/kanpyo_oracle.c vs the naive oracle/pyref.py) -- the only
token-level cross-check available while the reference cannot be built: >= 10 000 random sentences
over random small dictionaries with negative costs, missing unk entries, every invoke/group permutation,
duplicate surfaces, nested prefixes, non-BMP characters and dead ends.  CPU only."""
import numpy as np
import pytest

from lattice_cases import _random_dict, _sentence
from oracle import oracle, pyref


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_pyref_and_c_oracle_agree(seed):
    rng = np.random.default_rng(seed)
    total = 0
    for _ in range(50):
        d = _random_dict(rng, int(rng.integers(1, 6)))
        parts = (d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
        o = oracle.OracleTokenizer(*parts)
        p = pyref.PyDict(*parts)
        for _ in range(55):
            s = _sentence(rng)
            exp = pyref.tokenize(p, s)
            got, _ctr = o.tokenize(s)
            assert [tuple(int(x) for x in t) for t in got] == exp, (seed, s)
            total += 1
    assert total >= 2500  # x 4 seeds = 11 000 sentences


@pytest.mark.parametrize("seed", [11, 12])
def test_pyref_and_c_oracle_agree_on_keys_of_every_utf8_width(seed):
    """synth.width_case (1- to 4-byte characters and U+FFFF anywhere in a key): the dictionaries the gpu tests use to pin the device's
    character-level trie walk -- here the two CPU restatements of the byte-level walk (trie/da.rs:155-182) against each other."""
    import random

    from kanpyo_amd import synth

    rng = random.Random(seed)
    total = 0
    for _ in range(12):
        d, sents = synth.width_case(rng)
        parts = (d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
        o = oracle.OracleTokenizer(*parts)
        p = pyref.PyDict(*parts)
        for s in sents[:40]:
            s = s[:60]
            exp = pyref.tokenize(p, s)
            got, _ctr = o.tokenize(s)
            assert [tuple(int(x) for x in t) for t in got] == exp, (seed, s)
            total += 1
    assert total >= 200


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_pyref_and_c_oracle_agree_on_non_square_matrices(seed):
    """synth.matrix_case (rows != cols both ways, right ids >= rows with the flat index in range, an axis of 65 536 or more, i16
    extreme and tied costs): ConnectionTable::get(right, left) = data[rows * left + right] (connection.rs:12-14) in both CPU
    restatements.  The sentences stay short (|dp| far below 2^31: the C oracle's i32 sum must not overflow)."""
    import random

    from kanpyo_amd import synth

    rng = random.Random(seed)
    total, seen = 0, set()
    for _ in range(40):
        d, sents, meta = synth.matrix_case(rng)
        seen.add((meta["ranked"], (meta["rows"] > meta["cols"]) - (meta["rows"] < meta["cols"])))
        parts = (d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
        o = oracle.OracleTokenizer(*parts)
        p = pyref.PyDict(*parts)
        assert (p.row, p.col) == (meta["rows"], meta["cols"])
        for s in sents[:30]:
            s = s[:24]
            exp = pyref.tokenize(p, s)
            got, _ctr = o.tokenize(s)
            assert [tuple(int(x) for x in t) for t in got] == exp, (seed, meta, s)
            total += 1
    assert total >= 680  # x 3 seeds > 2000 sentences
    assert {r for r, _ in seen} == {True, False} and {1, -1} <= {o for _, o in seen}, seen
