"""The WordPiece matcher on the device (kgpu_wordpiece.hip: k_wordpiece_len, k_wordpiece_write<SPANS>; table_lookup and entry_equals of
kgpu_records_dev.h) on lists and words CHOSEN AGAINST IT (tests/wordpiece_cases.py, tests/table_keys.py): prefixes that collide with listed entries in
the full 32-bit hash, at equal and at unequal length; the same bytes in both tables; a probe chain that wraps the continuation table's end; words as
long as each table's longest entry and one character longer; max_word_chars from both sides with characters of 1 to 4 bytes; a window of 64 x 1024
ids; random lists over a small alphabet, with records that start inside a character; and a batch that sends every wavefront round the grid-stride
loop a second time.

Nothing is tokenized: every input is crafted records, and every word an unknown-class surface record, so the device matches it in the text.  Every
expected value comes from tests/encode_spans_ref.py (which asserts that its ids and offsets are tests/wordpiece_ref.py's); comparisons are exact, on
the whole buffers with the sentinels behind them, ragged and padded, without spans and with spans (the span checks of tests/test_gpu_encode_spans.py
run kgpu_encode_device on the same buffers and compare its bytes).  Every test first asserts, by the reference alone, that its case is what it
claims to be (wordpiece_cases.claim_*); tests/test_wordpiece_cpu.py runs the same cases through the host split."""
import numpy as np
import pytest

import encode_ref as E
import encode_spans_ref as S
import wordpiece_cases as WC
from record_cases import SENTINEL, SMALL_KEYS, _Dev, dev_encode, ref_spec, small_ctx, small_env  # noqa: F401  (small_ctx, small_env: the fixtures)
from record_cases import check_spans_padded as check_padded
from record_cases import check_spans_ragged as check_ragged

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 7, 64)


def reference(env, recs, case):
    """-> (ids, id_offsets, spans, token_index) of the records by the list, prefix and limit of `case`."""
    return S.encode(*recs, env.known, env.unk, env.nk, env.nu, ref_spec(), SMALL_KEYS, case.vocab, WC.UNK, wordpiece=True, prefix=case.prefix, max_chars=case.max_chars)


def cuts(want, width):
    """Where a row of `width` is cut, by the reference's token indices: "between" two tokens or "inside" a token's pieces, over the sentences that are cut."""
    off, tix = want[1].astype(np.int64), want[3]
    kinds = set()
    for s in np.flatnonzero(np.diff(off) > width).tolist():
        kinds.add("inside" if tix[off[s] + width] == tix[off[s] + width - 1] else "between")
    return kinds


def handle(env, case):
    return env.words().vocabulary(case.vocab, WC.UNK, wordpiece=True, prefix=case.prefix, max_word_chars=case.max_chars)


def run(env, ctx, case, recs=None, widths=WIDTHS, info=None, want=None):
    """The case ragged and padded, without spans and with them -> the kinds of cut its padded rows had.  info: what wordpiece_info must say."""
    recs = WC.records(case.sentences) if recs is None else recs
    want = reference(env, recs, case) if want is None else want
    v = handle(env, case)
    if info:
        wi = v.wordpiece_info()
        assert {k: wi[k] for k in info} == info, case
    d = _Dev(recs)
    check_ragged(ctx, v, d, want, what=case.name)
    kinds = set()
    for width in widths:
        kinds |= cuts(want, width)
        check_padded(ctx, v, d, want, width, None)
    v.close()
    return kinds


def bounds(case):
    """max_initial_bytes and max_cont_bytes, from the list."""
    cont = [len(w) for w in case.tables()[1]] if case.prefix else [len(w) for w in case.vocab]
    return {"max_initial_bytes": max(len(w) for w in case.vocab), "max_cont_bytes": max(cont, default=0), "cont_words": len(cont)}


# ---- A. colliding prefixes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["dead", "split"])
def test_a_prefix_with_the_hash_and_length_of_a_listed_twin(small_env, small_ctx, variant):
    case, trios = WC.twin_cases()[variant]
    WC.claim_twin(case, trios)
    assert run(small_env, small_ctx, case) == {"between", "inside"}


def test_both_keys_of_a_colliding_pair_listed(small_env, small_ctx):
    case, pairs = WC.both_listed_case()
    WC.claim_both_listed(case, pairs)
    assert run(small_env, small_ctx, case) == {"between", "inside"}


@pytest.mark.parametrize("variant", range(4), ids=["long", "long+pieces", "short", "short+pieces"])
def test_a_prefix_with_the_hash_of_an_entry_of_another_length(small_env, small_ctx, variant):
    case, asked = WC.cross_length_cases()[variant]
    assert case.name == "cross-" + ["long", "long+pieces", "short", "short+pieces"][variant]
    WC.claim_cross(case, asked)
    assert run(small_env, small_ctx, case) == {"between", "inside"}


@pytest.mark.parametrize("variant", [0, 1], ids=["two-tables", "one-shared-table"])
def test_the_same_bytes_in_both_tables(small_env, small_ctx, variant):
    case, keys = WC.both_tables_cases()[variant]
    assert bool(case.prefix) == (variant == 0)
    WC.claim_both_tables(case, keys)
    assert run(small_env, small_ctx, case, info=bounds(case)) == {"between", "inside"}


def test_a_wrapped_chain_in_the_continuation_table(small_env, small_ctx):
    one, rotated, keys = WC.chain_cases()
    WC.claim_chain(one, rotated, keys)
    info = {"cont_words": 8, "cont_table_slots": 16}
    assert run(small_env, small_ctx, one, widths=(1, 2, 64, 65, 100), info=info) == {"between", "inside"}
    assert run(small_env, small_ctx, rotated, widths=(2, 7), info=info) == {"between", "inside"}


# ---- B. the tables' longest entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5), ids=["initial-24", "cont-24", "inside-@", "inside-##", "no-cont"])
def test_the_tables_longest_entries(small_env, small_ctx, k):
    case = WC.longest_entry_cases()[k]
    WC.claim_longest(case)
    info = bounds(case)
    assert (info["max_initial_bytes"], info["max_cont_bytes"]) == [(24, 3), (26, 24), (4, 3), (5, 3), (3, 0)][k]
    kinds = run(small_env, small_ctx, case, info=info)
    assert kinds == ({"between"} if case.name == "no-cont" else {"between", "inside"})


# ---- C. max_word_chars from both sides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", WC.LIMITS)
def test_max_word_chars_from_both_sides(small_env, small_ctx, limit):
    case, count = WC.limit_case(limit)
    recs = WC.records(case.sentences)
    want = reference(small_env, recs, case)
    # (the reference's split of a 4096-byte word costs a second: what the claim reads is taken from `want`, every word's ids by its token index)
    ids, tix = want[0][: int(want[1][1])].tolist(), want[3][: int(want[1][1])].tolist()
    case.adopt({w: [i for i, t in zip(ids, tix) if t == k] for k, w in enumerate(case.sentences[0])})
    WC.claim_limit(case, count, limit)
    kinds = run(small_env, small_ctx, case, recs, widths=sorted({1, 2, 3, limit, limit + 1, 3 * limit}), want=want)
    assert kinds == ({"between"} if limit == 1 else {"between", "inside"})


def test_a_window_of_64_times_1024_ids(small_env, small_ctx):
    case = WC.full_window_case()
    WC.claim_full_window(case)
    recs = WC.full_window_records(case)
    want = reference(small_env, recs, case)
    assert len(recs[1]) == 2 and len(recs[2]) == 64 and len(want[0]) == 64 * 1024, "one sentence, one window: the bound k_wordpiece_write's comment states"
    assert want[3].tolist() == [k for k in range(64) for _ in range(1024)] and want[2][1024 + 5].tolist() == [20, 4, 5, 6], "every piece its own bytes and characters"
    kinds = run(small_env, small_ctx, case, recs, widths=(1, 1024, 1025, 65535), want=want)
    assert kinds == {"between", "inside"}


# ---- D. random lists over a small alphabet ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", WC.RANDOM_LIMITS)
@pytest.mark.parametrize("prefix", WC.PREFIXES, ids=["hashes", "at", "none", "eight-bytes"])
def test_random_lists(small_env, small_ctx, prefix, limit):
    case = WC.random_case(prefix, limit)
    WC.claim_random(case)
    assert run(small_env, small_ctx, case, widths=(1, 5, 64, 300)) == {"between", "inside"}
    # the same words with every record's bounds one byte later: words that begin with 10xxxxxx bytes, and that end inside a character
    recs = WC.records(case.sentences, shift=True)
    words = [w for s in WC.record_words(recs) for w in s]
    assert sum(1 for w in words if w and w[0] & 0xC0 == 0x80) >= 100 and sum(1 for w in words if w and w[0] & 0xC0 != 0x80) >= 100
    want = reference(small_env, recs, case)
    assert 0 < int((want[0] == WC.UNK).sum()) < len(want[0])
    assert run(small_env, small_ctx, case, recs, widths=(2, 64), want=want) == {"between", "inside"}


# ---- E. second trips of the grid-stride loops ------------------------------------------------------------------------------------------------------------------------
def test_second_trips_of_the_grid_stride_loops(small_env, small_ctx):
    n = WC.SECOND_TRIP_N
    assert n > WC.GRID_BLOCKS * WC.render_wpb(), "more sentences than the capped grid has wavefronts"
    recs = WC.second_trip_records(small_env.nk, small_env.nu)
    case = WC.Case("second-trips", WC.second_trip_list(), [])
    stats = {}
    want = S.encode(*recs, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(), SMALL_KEYS, case.vocab, WC.UNK, wordpiece=True, stats=stats)
    per = np.diff(recs[3].astype(np.int64))
    assert len(per) == n and all(per[s] == 200 for s in WC.LONG_AT) and per.max() == 200 and sorted(set(per.tolist())) == [0, 1, 2, 3, 200]
    assert stats["text_split"] > 1000 and stats["whole_split"] > 1000 and stats["row_split"] > 100 and stats["unk"] > 1000, stats
    L = np.diff(want[1].astype(np.int64))
    assert all(L[s] > 64 for s in WC.LONG_AT) and (L[WC.GRID_BLOCKS * WC.render_wpb():] > 0).sum() > 100, "ids in the second trip"
    v = handle(small_env, case)
    d = _Dev(recs)
    check_ragged(small_ctx, v, d, want)   # (with spans, and the plain call on the same buffers)
    width = 9
    assert cuts(want, width) == {"between", "inside"}
    ref = E.padded(want[0], want[1], width, -9)
    rc, got, buf, ioff = dev_encode(small_ctx, v, d, width=width, pad_id=-9, capacity=n * width, room=n * width + 48)
    assert (rc, got) == (0, len(want[0])) and np.array_equal(ioff, want[1])
    assert np.array_equal(buf[: n * width].reshape(n, width), ref) and (buf[n * width:] == SENTINEL).all()
    v.close()
