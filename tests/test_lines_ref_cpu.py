"""tests/lines_ref.py -- the reference renderer the GPU tests of kgpu_format.hip compare with -- pinned on the CPU: against the per-token
loop tests/test_gpu_lines.py compares with (lines_ref.expected_lines, which stays as it is), against the hand-derived lines of tests/golden/fixture_tokens.json,
and on every generator tests/test_gpu_format.py uses (each kind of crafted record, the window regimes, the 70 001-sentence shape and the
4 GiB shape scaled down to a few MiB)."""
import numpy as np
import pytest

import lines_ref as R
from conftest import load_golden
from lines_ref import expected_lines


def _small_tables():
    """The display tables of test_gpu_lines.py::test_edge_cases: known rows of 0, 62 and 10 200 bytes, an unknown row, an empty-string name."""
    from kanpyo_amd.dictfile import MorphFeatureTable

    k = MorphFeatureTable([[], [1, 0, 1], [2]], ["", "名" * 10, "長" * 3400])
    u = MorphFeatureTable([[1]] * 4, ["", "未知"])
    return k, u, R.rows_of(k, 3), R.rows_of(u, 4)


@pytest.fixture(scope="module")
def small():
    return _small_tables()


@pytest.fixture(scope="module")
def synth_tables():
    from kanpyo_amd import synth

    sd = synth.build_dict()
    k, u = synth.feature_tables(sd)
    return k, u, R.rows_of(k, len(k.morph_features)), R.rows_of(u, len(u.morph_features))


def _both(case, tables):
    k, u, krows, urows = tables
    utf8, offsets, tokens, tok_offsets = case
    want, want_off = expected_lines(utf8, offsets, tokens, tok_offsets, k, u)
    got, got_off = R.render(utf8, offsets, tokens, tok_offsets, krows, urows)
    assert got_off.dtype == np.uint64 and np.array_equal(got_off, want_off)
    assert got == want
    lens = R.line_lengths(utf8, offsets, tokens, tok_offsets, krows, urows)
    assert int(lens.sum()) == len(want) and (lens >= 2).all()
    return got, got_off


def test_token_dtype_is_the_librarys():
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    assert R.TOKEN_DTYPE == TOKEN_DTYPE and R.TOKEN_DTYPE.itemsize == 24


def test_small_rows_have_the_lengths_the_tests_name(small):
    _, _, krows, urows = small
    assert [len(r) for r in krows] == [0, 62, 10200] and urows[0] == "未知".encode()


def test_fixture_tokens_hand_derived():
    """The lines of tests/golden/fixture_tokens.json, built the way test_gpu_lines.py::test_fixture_dictionary_hand_derived builds them."""
    cases = load_golden("fixture_tokens.json")["cases"]
    n_known = max(t[0] for c in cases for t in c["tokens"] if t[1] == 1)
    n_unk = max(t[0] for c in cases for t in c["tokens"] if t[1] == 2)
    krows = [f"名詞,k{i},*".encode() for i in range(1, n_known + 1)]
    urows = [f"未知語,u{i}".encode() for i in range(1, n_unk + 1)]
    want, want_off = b"", [0]
    for c in cases:
        for tid, cls, _pos, _start, _end, surface in c["tokens"]:
            feats = "" if cls == 0 or tid == 0 else (f"名詞,k{tid},*" if cls == 1 else f"未知語,u{tid}")
            want += f"{surface}\t{feats}\n".encode()
        want_off.append(len(want))
    case = R.pack([c["input"].encode() for c in cases],
                  [[(tid, cls, pos, len(surface.encode()) if cls else 0) for tid, cls, pos, _s, _e, surface in c["tokens"]] for c in cases])
    got, got_off = R.render(*case, krows, urows)
    assert got == want and got_off.tolist() == want_off
    assert any(not c["tokens"] for c in cases) and b"EOS\t\n" in got


@pytest.mark.parametrize("kind", R.KINDS)
def test_each_kind_of_record(small, synth_tables, kind):
    for tables, seed in ((small, 1), (synth_tables, 2)):
        rng = np.random.default_rng([seed, R.KINDS.index(kind)])
        case = R.make_records(rng, 300, (0, 5), [kind], len(tables[2]), len(tables[3]), known_ids=[1, 2] if tables is small else None)
        text, off = _both(case, tables)
        assert off[-1] == len(text) > 0
    utf8, offsets, tokens, tok_offsets = case
    B = np.diff(offsets.astype(np.int64))[np.repeat(np.arange(300), np.diff(tok_offsets.astype(np.int64)))]
    has = {
        "known": lambda t: (t["cls"] == 1).all() and (t["id"] >= 1).all(),
        "known_edge": lambda t: set(t["id"].tolist()) == {1, len(tables[2])},
        "unk": lambda t: (t["cls"] == 2).all() and (t["id"] >= 1).all(),
        "unk_edge": lambda t: set(t["id"].tolist()) == {1, len(tables[3])} and (t["cls"] == 2).all(),
        "known0": lambda t: (t["cls"] == 1).all() and (t["id"] == 0).all(),
        "dummy": lambda t: (t["cls"] == 0).all() and (t["id"] == 0).all(),
        "dummy_id": lambda t: (t["cls"] == 0).all() and (t["id"] != 0).all() and (t["id"] < 0).any(),
        "empty0": lambda t: (t["position"] == 0).all() and (t["byte_len"] == 0).all(),
        "emptyB": lambda t: (t["position"] == B).all() and (t["byte_len"] == 0).all() and (B > 0).any(),
        "overlap": lambda t: (t["position"] == 0).all() and (t["byte_len"] == B).all(),
        "backwards": lambda t: (np.diff(t["position"].astype(np.int64)) < 0).any(),
    }[kind]
    assert has(tokens), "the generator did not draw what the kind names"


def test_every_kind_mixed_with_empty_sentences(small, synth_tables):
    for tables, ids in ((small, [1, 2, 2, 2, 3]), (synth_tables, None)):
        rng = np.random.default_rng(5)
        case = R.make_records(rng, 2000, (0, 6), R.KINDS, len(tables[2]), len(tables[3]), known_ids=ids)
        _, off = _both(case, tables)
        nbytes, ntok = np.diff(case[1].astype(np.int64)), np.diff(case[3].astype(np.int64))
        assert (nbytes == 0).any() and (ntok == 0).any() and ((nbytes == 0) & (ntok > 0)).any()
        assert (np.diff(off.astype(np.int64))[ntok == 0] == 0).all()   # a sentence without tokens renders to nothing


@pytest.mark.parametrize("regime", ["two", "cycle", "big"])
def test_window_regimes(small, regime):
    for T in R.WINDOW_TOKENS:
        text, off = _both(R.window_case(regime, T), small)
        lens = R.line_lengths(*R.window_case(regime, T), small[2], small[3])
        assert lens.size == T and off.tolist() == [0, len(text)]
        if regime == "two":
            assert (lens == 2).all() and text == b"\t\n" * T
        elif regime == "cycle" and T >= 39:
            assert set(lens.tolist()) == set(range(2, 41))
        elif regime == "big" and T:
            assert set(lens[::3].tolist()) <= set(range(10203, 10208)) and (np.delete(lens, np.s_[::3]) == 2).all()


def test_window_starts_fall_on_every_offset_of_a_unit(small):
    """The coverage test 2 of test_gpu_format.py asserts on the device run, from the reference's own line lengths: over the 'cycle' set and the four
    misalignments, the first byte of a window behind a sentence's first falls on each of the 16 offsets of an address-aligned unit."""
    seen = set()
    for T in R.WINDOW_TOKENS:
        lens = R.line_lengths(*R.window_case("cycle", T), small[2], small[3])
        starts = np.concatenate([[0], np.cumsum(lens)])[64:T:64]
        seen |= {int(s + mis) % 16 for s in starts for mis in R.WINDOW_MIS}
    assert seen == set(range(16))


def test_many_sentences_shape(synth_tables):
    nk, nu = len(synth_tables[2]), len(synth_tables[3])
    rng = np.random.default_rng(70001)
    case = R.many_case(rng, 70001, nk, nu, long_at=(0, 32768, 70000))
    _, off = _both(case, synth_tables)
    ntok = np.diff(case[3].astype(np.int64))
    assert ntok[0] == ntok[32768] == ntok[70000] == 200 and (ntok == 0).mean() > 0.4
    for n in (0, 1, 255):
        _both(R.many_case(np.random.default_rng(n), n, nk, nu), synth_tables)


def test_the_4gib_shape_scaled_down(small):
    """big_case with a few hundred records: about 4 MiB through both renderers, and the column layout the device test checks."""
    rng = np.random.default_rng(4)
    counts = np.array([40, 300, 0, 70])
    case = R.big_case(rng, counts)
    text, off = _both(case, small)
    T = int(counts.sum())
    assert len(text) == T * 10203 and np.array_equal(off, np.concatenate([[0], np.cumsum(counts * 10203)]).astype(np.uint64))
    v = np.frombuffer(text, dtype=np.uint8).reshape(T, 10203)
    idx = np.concatenate([np.arange(c) for c in counts])
    sent = np.repeat(np.arange(4), counts)
    assert np.array_equal(v[:, 0], case[0][sent * 251 + idx % 251])
    assert (v[:, 1] == 9).all() and (v[:, -1] == 10).all() and (v[:, 2:10202] == np.frombuffer(small[2][2], dtype=np.uint8)).all()


def test_records_the_tokenizer_could_not_write_are_refused(small):
    """render() is for valid records only: it raises where the reference would panic, so a test cannot compare with a clipped slice by accident."""
    _, _, krows, urows = small
    for rec in [(4, 1, 0, 1), (-1, 1, 0, 1), (1, 3, 0, 1), (1, 1, 5, 0), (1, 1, 2, 3), (5, 2, 0, 0)]:
        with pytest.raises(ValueError):
            R.render(*R.pack([b"abcd"], [[rec]]), krows, urows)
    utf8, offsets, tokens, _ = R.pack([b"abcd", b"ef"], [[(1, 1, 0, 1)], [(1, 1, 0, 1)]])
    with pytest.raises(ValueError):
        R.render(utf8, offsets, tokens, np.array([1, 0, 2], dtype=np.uint64), krows, urows)
