"""Known answers for connection matrices that are not square and costs at the i16 extremes, in both CPU restatements
(oracle/kanpyo_oracle.c and oracle/pyref.py).  ConnectionTable::get(right, left) = data[rows * left + right]
(connection.rs:12-14); the Viterbi total is (dp + cost + matrix).min(INF) with a strict '<' against INF, and the
backtrace stops at the first node without a predecessor (lattice.rs:116-150).  The same dictionaries run on the GPU in
tests/test_gpu_matrix.py.  CPU only."""
import pytest

from dict_cases import saturation_parts, transposed_parts
from kanpyo_amd.dict import Dict
from oracle import oracle, pyref

INF = 1 << 30
A, I = "あ", "い"


def saturation_expected(n, m):
    """n あ then m い, derived by hand.  dp(あ_k) = 32767 + (k - 1) * 65534 = 65534 k - 32767, below INF up to k = 16385
    (INF - 1) and saturated from k = 16386 on: INF, no predecessor (the total is not < INF).  い_1 after a saturated あ:
    INF - 65536 < INF, so it takes あ_n as predecessor and the path is alive again -- but the backtrace from EOS stops at
    あ_n, which has none: only the い and EOS are returned.  Without い, EOS itself stays at INF: no path at all.
    -> (record count, first record)"""
    sat = n >= 16386
    if sat and m == 0:
        return 0, None
    if sat:
        return m + 1, (2, 1, 3 * n, n, n + 1, 3)
    return n + m + 1, ((1, 1, 0, 0, 1, 3) if n else (2, 1, 0, 0, 1, 3))


def _both(d, text):
    o = oracle.OracleTokenizer.from_dict(d)
    p = pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
    got, _ = o.tokenize(text)
    got = [tuple(int(x) for x in t) for t in got]
    assert got == pyref.tokenize(p, text), text[:8]
    return got


def test_saturation_boundary_is_where_the_hand_derivation_puts_it():
    assert 65534 * 16385 - 32767 == INF - 1 and 65534 * 16386 - 32767 >= INF


@pytest.mark.parametrize("n", [16383, 16384, 16385, 16386, 17000])
@pytest.mark.parametrize("m", [0, 3, 5])
def test_saturated_dp_and_truncated_backtrace(n, m):
    d = Dict.from_parts(**saturation_parts())
    got = _both(d, A * n + I * m)
    count, first = saturation_expected(n, m)
    assert len(got) == count
    if count:
        assert got[0] == first
        assert got[-1] == (0, 0, 3 * (n + m), n + m, n + m + 3, 0)   # EOS
        if m:
            assert all(t[0] == 2 for t in got[-m - 1 : -1])
        assert [t[3] for t in got[:-1]] == list(range(n + m - count + 1, n + m))   # one node per character, in order


def test_saturation_short_sentences():
    """The same dictionary far from saturation: every step is exact i16 arithmetic."""
    d = Dict.from_parts(**saturation_parts())
    assert _both(d, A + I) == [(1, 1, 0, 0, 1, 3), (2, 1, 3, 1, 2, 3), (0, 0, 6, 2, 5, 0)]
    assert _both(d, I * 4) == [(2, 1, 3 * k, k, k + 1, 3) for k in range(4)] + [(0, 0, 12, 4, 7, 0)]
    assert _both(d, "") == [(0, 0, 0, 0, 3, 0)]


def test_rows_not_cols_decides_the_token():
    d = Dict.from_parts(**transposed_parts())
    assert _both(d, A + I) == [(2, 1, 0, 0, 1, 3), (3, 1, 3, 1, 2, 3), (0, 0, 6, 2, 5, 0)]
    assert _both(d, A + I + A + I) == [(2, 1, 0, 0, 1, 3), (3, 1, 3, 1, 2, 3), (2, 1, 6, 2, 3, 3), (3, 1, 9, 3, 4, 3), (0, 0, 12, 4, 7, 0)]
    # あ at the end: its next node is EOS, get(right, 0) = data[0] for id 1 and data[2] = -500 for id 2
    assert _both(d, A)[0] == (2, 1, 0, 0, 1, 3)


def test_flat_index_beyond_rows_is_the_reference_behaviour():
    """right_id >= rows with rows * left + right inside the matrix: no panic, the flat element is read (connection.rs:13)."""
    p = transposed_parts()
    p["morphs"] = [[0, 4, 0], [0, 2, 0], [0, 0, 0]]   # id 1: right 4 >= rows 3; every left is 0, so the flat index stays below 6
    p["conn_data"] = [0, 0, 0, 0, -300, -200]
    # id 1 -> い reads data[4] = -300, id 2 -> い reads data[2] = 0: id 1 wins; EOS after い: data[0]
    assert _both(Dict.from_parts(**p), A + I) == [(1, 1, 0, 0, 1, 3), (3, 1, 3, 1, 2, 3), (0, 0, 6, 2, 5, 0)]
