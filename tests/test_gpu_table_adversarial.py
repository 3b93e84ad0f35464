"""The byte-keyed table of the word counts and the vocabulary ids (kgpu_count.hip, kgpu_encode.hip, kgpu_records_dev.h) and the count kernel's
LDS row table on keys CHOSEN AGAINST THEM (tests/table_keys.py): different words with one full 32-bit hash, probe chains that wrap the table's
end and are inserted by many wavefronts in different orders, a workgroup's row table with more rows than entries, and all of it in one launch.
Every case is legal input under the header's contract.  Expected values come from count_ref / encode_ref on the crafted records alone, entry
for entry; there is no tolerance.  Every test first asserts, by the reference alone, that its case is what it is meant to be."""
import threading
from collections import Counter

import numpy as np
import pytest

import count_ref as CR
import encode_ref as E
import lines_ref as R
import table_keys as T
import words_ref as W
from record_cases import (SENTINEL, _Dev, check_ragged, crafted_ids, crafted_want, dev_count, dev_encode, holds, ref_spec, small_ctx,  # noqa: F401
                          small_env, synth_env)   # (small_ctx, small_env: the fixtures)

pytestmark = pytest.mark.gpu

U, K = R.UNKNOWN, R.KNOWN
UNK = -3


@pytest.fixture(scope="module")
def env():
    """The 20 000-record dictionary with its display tables, its keys by id and a context that never tokenizes."""
    from kanpyo_amd.device import DeviceContext

    e = synth_env()
    e.ctx = DeviceContext(e.tok)
    yield e
    e.ctx.close()


def pairs():
    same, cross, big = T.adversarial_pairs()
    assert len(same) >= 8 and len(cross) >= 4 and len(big[0]) == len(big[1]) == 3072
    out = same + cross + [big]
    assert all(a != b and E.key_hash(a) == E.key_hash(b) for a, b in out)
    return out


def _laid_out(keys):
    """The keys back to back -> (text, {key: position})."""
    at, pos = 0, {}
    for k in keys:
        pos[k] = at
        at += len(k)
    return b"".join(keys), pos


# ---- the crafted batches ---------------------------------------------------------------------------------------------------------------------------
def one_wavefront_case(ps):
    """One sentence.  Its first window holds the two keys of every pair in ADJACENT LANES (both new, one hash, one home slot: one of them loses the
    claiming swap to a different word); behind it 2 more of every a and 4 more of every b, shuffled: 3 and 5 overall."""
    text, pos = _laid_out([k for p in ps for k in p])
    assert 2 * len(ps) <= 64
    recs = [(j % 2, U, pos[k], len(k)) for j, k in enumerate(k for p in ps for k in p)]
    rest = [k for a, b in ps for k in (a, a, b, b, b, b)]
    order = np.random.default_rng(3).permutation(len(rest))
    recs += [(int(j) % 2, U, pos[rest[j]], len(rest[j])) for j in order]
    return R.pack([text], [recs])


def across_wavefronts_case(ps, n=64):
    """n sentences; sentence s holds the two keys of pair s mod P twice each, a first when s is even and b first when s is odd."""
    sents, recs = [], []
    for s in range(n):
        a, b = ps[s % len(ps)]
        x, y = (a, b) if s % 2 == 0 else (b, a)
        sents.append(x + y)
        recs.append([(0, U, 0, len(x)), (1, U, len(x), len(y)), (1, U, 0, len(x)), (0, U, len(x), len(y))])
    return R.pack(sents, recs)


def rotated_case(words, n=256):
    """n sentences, each holding all the words once, rotated by s: the wavefronts meet the same new words in different orders."""
    L = len(words[0])
    assert all(len(w) == L for w in words)
    sents = [b"".join(words[s % len(words):] + words[: s % len(words)]) for s in range(n)]
    return R.pack(sents, [[(j % 2, U, L * j, L) for j in range(len(words))]] * n)


def recs_of(case, s):
    """The records of sentence s of a packed case."""
    return case[2][int(case[3][s]): int(case[3][s + 1])]


def surfaces_case(per_sentence):
    """Per sentence a list of keys -> unknown-class records over the keys back to back."""
    sents, recs = [], []
    for keys in per_sentence:
        sents.append(b"".join(keys))
        at, r = 0, []
        for j, k in enumerate(keys):
            r.append((j % 2, U, at, len(k)))
            at += len(k)
        recs.append(r)
    return R.pack(sents, recs)


# ---- A. colliding keys, counts ----------------------------------------------------------------------------------------------------------------------
def _pair_counter(small_env):
    return small_env.words().counter(table_slots=64, key_bytes=1 << 16)


def test_colliding_keys_count_in_one_wavefront(small_env, small_ctx):
    ps = pairs()
    case = one_wavefront_case(ps)
    want = crafted_want(small_env, case, {})
    assert len(want) == 2 * len(ps) and all(want[a] == 3 and want[b] == 5 for a, b in ps), "both keys of every pair, apart"
    first = case[2][:64]
    assert all(bytes(case[0][int(first["position"][2 * p]):][: len(a)]) == a and bytes(case[0][int(first["position"][2 * p + 1]):][: len(b)]) == b
               for p, (a, b) in enumerate(ps)), "the two keys of a pair are neighbours in the first window"
    k = _pair_counter(small_env)
    assert dev_count(small_ctx, k, case) == (0, 8 * len(ps))
    info = holds(k, want)
    assert info["table_slots_used"] == len(want)
    k.close()


def test_colliding_keys_count_across_wavefronts(small_env, small_ctx):
    ps = pairs()
    case = across_wavefronts_case(ps)
    want = crafted_want(small_env, case, {})
    assert len(want) == 2 * len(ps) and all(want[a] == want[b] >= 6 for a, b in ps)
    firsts = {bytes(case[0][int(case[1][s]):][: int(case[2]["byte_len"][4 * s])]) for s in range(64)}
    assert all(a in firsts and b in firsts for a, b in ps), "every key comes first in some sentence"
    k = _pair_counter(small_env)
    assert dev_count(small_ctx, k, case) == (0, 256)
    info = holds(k, want)
    assert info["table_slots_used"] == len(want)
    k.close()


def test_colliding_keys_count_into_a_warm_table(small_env, small_ctx):
    ps = pairs()
    warm = surfaces_case([[a for a, _ in ps]])
    want = crafted_want(small_env, warm, {})
    assert want == Counter({a: 1 for a, _ in ps})
    k = _pair_counter(small_env)
    assert dev_count(small_ctx, k, warm) == (0, len(ps))
    assert holds(k, want)["table_slots_used"] == len(ps)
    for case in (one_wavefront_case(ps), across_wavefronts_case(ps)):   # every b now meets its partner's slot occupied
        crafted_want(small_env, case, {}, into=want)
        assert dev_count(small_ctx, k, case)[0] == 0
        assert len(want) == 2 * len(ps)
        assert holds(k, want)["table_slots_used"] == len(want)
    k.close()


# ---- B. colliding keys, encode ----------------------------------------------------------------------------------------------------------------------
def _neighbours(ids, x, y):
    ids = np.asarray(ids)
    return bool(((ids[:-1] == x) & (ids[1:] == y)).any() or ((ids[:-1] == y) & (ids[1:] == x)).any())


@pytest.mark.parametrize("listed", ["a", "b", "both"])
def test_colliding_keys_encode(small_env, small_ctx, listed):
    ps = pairs()
    head = [b"<pad>", b"<s>"]
    vocab = head + {"a": [a for a, _ in ps], "b": [b for _, b in ps], "both": [k for p in ps for k in p]}[listed]
    index = {w: i for i, w in enumerate(vocab)}
    v = small_env.words().vocabulary(vocab, UNK)
    for case in (one_wavefront_case(ps), across_wavefronts_case(ps)):
        want = crafted_ids(small_env, case, {}, vocab, UNK)
        for a, b in ps:   # by the reference alone: the partners are neighbours, with different ids
            ia, ib = index.get(a, UNK), index.get(b, UNK)
            assert ia != ib and (ia == UNK) == (listed == "b") and (ib == UNK) == (listed == "a")
            assert _neighbours(want[0], ia, ib), "a pair's keys never sit in neighbouring positions"
        assert (UNK in want[0]) == (listed != "both") and set(want[0].tolist()) - {UNK} == {index[k] for p in ps for k in p if k in index}
        dcase = _Dev(case)
        check_ragged(small_ctx, v, dcase, want)
        n = dcase.n
        for width in (1, 64):
            ref = E.padded(want[0], want[1], width, -9)
            rc, got, buf, ioff = dev_encode(small_ctx, v, dcase, width=width, pad_id=-9, capacity=n * width, room=n * width + 48)
            assert (rc, got) == (0, len(want[0])) and np.array_equal(ioff, want[1])
            assert np.array_equal(buf[: n * width].reshape(n, width), ref), (listed, width)
            assert (buf[n * width:] == SENTINEL).all(), "ids behind n x width"
    v.close()


# ---- C. wrapped chains ------------------------------------------------------------------------------------------------------------------------------
def test_wrapped_chain_counts(small_env, small_ctx):
    from kanpyo_amd import _lib

    words, more, covered = T.chain(64, 61, 48, absent=11)
    # (one key of EVERY home 0..10 would make 48 + 8 + 11 = 67 words: six of them, so that 62 fit and two more fill the 64 slots exactly)
    inside = covered[0:11:2]   # homes 0, 2, .. 10: inside the chain 61, 62, 63, 0, .. 44
    assert all(E.key_hash(w) & 63 == 61 for w in words + more) and [E.key_hash(w) & 63 for w in inside] == [0, 2, 4, 6, 8, 10]
    assert len(set(words + more + inside)) == 48 + 11 + 6
    case = rotated_case(words)
    want = crafted_want(small_env, case, {})
    assert want == Counter({w: 256 for w in words}) and len(want) == 48
    k = small_env.words().counter(table_slots=64, key_bytes=1 << 20)
    assert dev_count(small_ctx, k, case) == (0, 256 * 48)
    info = holds(k, want)
    assert info["table_slots_used"] == 48 and info["key_bytes_used"] >= 48 * 16   # (a word met by several wavefronts at once may take its 16 bytes twice)
    # 8 more of that home and 6 whose home the chain covers, among words that are there already, again in rotation
    second = more[:8] + inside + words[40:]
    case = surfaces_case([second[s:] + second[:s] for s in range(len(second))])
    crafted_want(small_env, case, {}, into=want)
    assert len(want) == 62
    assert dev_count(small_ctx, k, case) == (0, len(second) ** 2)
    assert holds(k, want)["table_slots_used"] == 62
    # exactly full
    case = surfaces_case([more[8:10] + words[:3], more[8:10][::-1]])
    crafted_want(small_env, case, {}, into=want)
    assert len(want) == 64
    assert dev_count(small_ctx, k, case) == (0, 7)
    assert holds(k, want)["table_slots_used"] == 64
    # full: a present key counts (the last of the chain, the first, one from inside), an absent one overflows -- and nothing else changes
    case = surfaces_case([[more[9], words[0], inside[3], more[9]]])
    crafted_want(small_env, case, {}, into=want)
    assert dev_count(small_ctx, k, case) == (0, 4)
    holds(k, want)
    absent = more[10]
    assert absent not in want and E.key_hash(absent) & 63 == 61
    case = surfaces_case([[words[5], absent, words[6]]])
    crafted_want(small_env, surfaces_case([[words[5], words[6]]]), {}, into=want)
    rc, counted = dev_count(small_ctx, k, case)
    assert rc == _lib.KGPU_ERR_CAPACITY and counted == 2
    info = holds(k, want, overflow=1)   # every reported count is the true one, reported + overflow = tokens kept, the order is rule 5's
    assert info["table_slots_used"] == 64 and info["overflow_tokens"] == 1 and len(k.most_common()) == 64
    k.close()


@pytest.mark.parametrize("slots, listed", [(16, 8), (64, 32)])
def test_wrapped_chain_encode(small_env, small_ctx, slots, listed):
    words, absent, covered = T.chain(slots, slots - 1, listed)
    assert all(E.key_hash(w) & (slots - 1) == slots - 1 for w in words + absent) and [E.key_hash(w) & (slots - 1) for w in covered] == list(range(listed - 1))
    v = small_env.words().vocabulary(words, UNK, 100, 101)
    assert v.info()["table_slots"] == slots and v.info()["n_words"] == listed
    mixed = [k for trio in zip(words, (absent * listed)[:listed], (covered + covered[:1])) for k in trio]
    case = surfaces_case([mixed, mixed[::-1], [], absent + words[-1:] + covered[-3:]])
    want = crafted_ids(small_env, case, {}, words, UNK, 100, 101)
    got = Counter(want[0].tolist())
    assert all(got[i] == 2 + (i == listed - 1) for i in range(listed)) and got[UNK] == 4 * listed + 4 + 3, "every listed word by its index, every absent one unk"
    dcase = _Dev(case)
    check_ragged(small_ctx, v, dcase, want)
    ref = E.padded(want[0], want[1], 64, -9, 101)
    rc, n_ids, buf, ioff = dev_encode(small_ctx, v, dcase, width=64, pad_id=-9, capacity=4 * 64, room=4 * 64 + 48)
    assert (rc, n_ids) == (0, len(want[0])) and np.array_equal(ioff, want[1])
    assert np.array_equal(buf[: 4 * 64].reshape(4, 64), ref) and (buf[4 * 64:] == SENTINEL).all()
    v.close()


# ---- D. the workgroup's row table --------------------------------------------------------------------------------------------------------------------
def known_case(per_sentence):
    """Known-class records with position 0 and byte_len 0 over one-byte sentences: by rule 2 the dictionary's key of the id is the word."""
    return R.pack([b"x"] * len(per_sentence), [[(int(i), K, 0, 0) for i in ids] for ids in per_sentence])


def d2_draw(s, n=600):
    """Sentence s of D2: n ids drawn from 1..2500 and 20 hot ids 50 times each, shuffled (fixed seeds)."""
    hot = np.random.default_rng(21).choice(2500, 20, replace=False) + 1
    rng = np.random.default_rng(100 + s)
    return rng.permutation(np.concatenate([rng.integers(1, 2501, n), np.repeat(hot, 50)])).tolist()


def _row_count(env, case, kw=None, want_slots=0):
    kw = kw or {}
    want = CR.count(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), env.keys)
    k = env.words(**kw).counter(table_slots=64, key_bytes=4096)
    assert dev_count(env.ctx, k, case) == (0, len(case[2]))
    info = holds(k, want)
    assert info["tokens_counted"] == len(case[2]) and info["table_slots_used"] == want_slots
    k.close()
    return want


def test_row_table_more_rows_than_entries(env):
    ids = list(range(1, 3001))
    case = known_case([ids + ids[::-1]])
    assert len(set(ids)) > T.LDS_ENTRIES
    want = _row_count(env, case)
    assert len(want) < 3000 and sum(want.values()) == 6000 and max(want.values()) > 2, "some ids share a surface: the read-out merges rows"


def test_row_table_eight_wavefronts_fill_it_together(env):
    per = [d2_draw(s) for s in range(8)]
    rows = {i for ids in per for i in ids}
    assert len(per) == 8 and len(rows) > T.LDS_ENTRIES and all(len(ids) == 1600 for ids in per)
    hot = Counter(i for ids in per for i in ids).most_common(20)
    assert hot[-1][1] >= 8 * 50, "twenty rows that every wavefront adds to throughout"
    want = _row_count(env, known_case(per))
    assert sum(want.values()) == 8 * 1600


def test_row_table_crowded_homes(env):
    homes = (1020, 1023, 300, 301)   # two pairs whose 8-entry probe ranges overlap, one of them around the table's end
    ids = []
    for h in homes:
        rows = T.rows_with_lds_home(env.nk, h)
        assert len(rows) >= 12 > T.LDS_PROBES + 1 and all(int(T.lds_home(r)) == h for r in rows), "at least 9 rows on a home"
        ids += [r + 1 for r in rows]
    assert len(set(ids)) == len(ids) >= 48
    want = _row_count(env, known_case([ids * 7]))
    assert sum(want.values()) == 7 * len(ids) and min(want.values()) >= 7


def test_row_table_known_and_unknown_rows(env):
    kw = {"field": 0}
    spec = ref_spec(**kw)
    known_ids = (np.random.default_rng(31).choice(2500, 1500, replace=False) + 1).tolist()
    unk_ids = list(range(1, env.nu + 1))
    unk_words = {W.row_word(env.unk.features(t), spec) for t in unk_ids}
    known_words = {W.row_word(env.known.features(t), spec) or env.keys[t - 1].encode() for t in known_ids}
    assert None not in unk_words, "every unknown row's word is a pool name: none goes to the byte table"
    assert unk_words - known_words and unk_words & known_words, "a pool name of the unknown rows alone, and one the known rows share"
    recs = [(i, K, 0, 0) for i in known_ids] + [(t, U, 0, 0) for t in unk_ids] * 40
    order = np.random.default_rng(32).permutation(len(recs))
    case = R.pack([b"x"], [[recs[j] for j in order]])
    assert len(known_ids) + env.nu > T.LDS_ENTRIES
    want = _row_count(env, case, kw)
    assert set(want) == unk_words | known_words and all(want[w] >= 40 for w in unk_words)


def test_row_table_second_sentence_of_a_wavefront(env):
    n = 2048 + 300   # 256 workgroups of 8 wavefronts: 300 wavefronts take a second sentence
    case = known_case([[(37 * s) % 1200 + 1] for s in range(n)])
    want = _row_count(env, case)
    assert sum(want.values()) == n


# ---- E. both tables at once ----------------------------------------------------------------------------------------------------------------------------
def e_known_ids(env, s):
    """The 200 known ids of sentence s of E: 180 drawn from 1..2500 (D2's draw, without its hot ids) and, shuffled among them, the first 10 rows of each
    of two first entries of the LDS table four apart -- the same 20 in all eight sentences of a workgroup (sentences 8 w .. 8 w + 7), so its eight wavefronts
    contend on them while their 8-entry probe ranges overflow."""
    w = s // 8
    crowd = [r + 1 for h in (100 * w + 7, 100 * w + 11) for r in T.rows_with_lds_home(env.nk, h)[:10]]
    rng = np.random.default_rng(100 + s)
    return rng.permutation(np.concatenate([rng.integers(1, 2501, 180), crowd])).tolist()


def test_both_tables_in_one_launch_and_the_round_trip(env):
    ps = pairs()
    cluster = T.keys_with_home(256, 253, 40, 6, 5)
    assert all(E.key_hash(w) & 255 == 253 for w in cluster)
    sents, recs = [], []
    for s in range(64):
        a_first = [k for a, b in ps for k in ((a, b) if s % 2 == 0 else (b, a))]
        text, pos = _laid_out(cluster[s % 40:] + cluster[: s % 40] + a_first)
        unknown = [(j % 2, U, pos[k], len(k)) for j, k in enumerate(pos)]
        known = [(int(i), K, 0, 0) for i in e_known_ids(env, s)]
        rng = np.random.default_rng(500 + s)
        slots = np.zeros(len(unknown) + len(known), dtype=bool)
        slots[rng.choice(len(slots), len(unknown), replace=False)] = True   # the unknown records keep their order among the known ones
        u, kn = iter(unknown), iter(known)
        sents.append(text)
        recs.append([next(u) if f else next(kn) for f in slots])
    case = R.pack(sents, recs)
    for w in range(8):   # by the records and lds_home alone: every workgroup's row table is over-full, with more rows on one first entry than a probe walks
        rows = {int(t["id"]) - 1 for ss in range(8 * w, 8 * w + 8) for t in recs_of(case, ss) if t["cls"] == K}
        per_home = Counter(T.lds_home(np.array(sorted(rows))).tolist())
        assert len(rows) > T.LDS_ENTRIES and max(per_home.values()) >= T.LDS_PROBES + 1, (w, len(rows), max(per_home.values()))
    want = CR.count(*case, env.known, env.unk, env.nk, env.nu, ref_spec(), env.keys)
    surfaces = set(cluster) | {k for p in ps for k in p}
    assert len(surfaces) == 40 + 2 * len(ps) and not surfaces & {w.encode() for w in env.keys} and all(want[w] == 64 for w in surfaces)
    assert sum(want.values()) == len(case[2]) == 64 * (200 + len(surfaces))
    k = env.words().counter(table_slots=256, key_bytes=1 << 20)
    assert dev_count(env.ctx, k, case) == (0, len(case[2]))
    info = holds(k, want)
    assert info["table_slots_used"] == len(surfaces)
    # every second distinct word listed, bos and eos
    order = [w for w, _ in CR.ordered(want)]
    vocab = [b"<s>", b"</s>", b"<unk>"] + order[::2]
    want_ids = E.encode(*case, env.known, env.unk, env.nk, env.nu, ref_spec(), env.keys, vocab, 2, 0, 1)
    listed = set(vocab)
    assert 0 < int((want_ids[0] == 2).sum()) < len(want_ids[0]) and surfaces & listed and surfaces - listed
    dcase = _Dev(case)
    v = env.words().vocabulary(vocab, 2, 0, 1)
    check_ragged(env.ctx, v, dcase, want_ids)
    v.close()
    # the round trip: the handle's own vocabulary; the ids' histogram is the counts, in list order
    v = k.vocabulary()
    assert v.words == [b"<pad>", b"<unk>"] + order and v.unk_id == 1
    total = len(case[2])
    rc, n_ids, buf, ioff = dev_encode(env.ctx, v, dcase, room=total + 32)
    assert (rc, n_ids) == (0, total)
    assert np.array_equal(np.bincount(buf[:total], minlength=len(v.words)), [0, 0] + [n for _, n in CR.ordered(want)])
    want_ids = E.encode(*case, env.known, env.unk, env.nk, env.nu, ref_spec(), env.keys, v.words, 1)
    assert np.array_equal(buf[:total], want_ids[0]) and np.array_equal(ioff, want_ids[1])
    v.close()
    k.close()


# ---- F. several contexts into one handle ------------------------------------------------------------------------------------------------------------
def test_eight_contexts_insert_one_chain_into_one_handle(small_env):
    """Rule 8: eight threads, each with a context of its own, add the rotated batch into one 64-slot handle at once.  Run once."""
    from kanpyo_amd.device import DeviceContext

    words, _, _ = T.chain(64, 61, 48, absent=11)
    case = rotated_case(words)
    want = Counter()
    for _ in range(8):
        crafted_want(small_env, case, {}, into=want)
    assert want == Counter({w: 8 * 256 for w in words})
    d = _Dev(case)
    k = small_env.words().counter(table_slots=64, key_bytes=1 << 22)
    ctxs = [DeviceContext(small_env.tok) for _ in range(8)]
    errors = []

    def work(t):
        try:
            ctxs[t].count_words(k, d.utf8.data_ptr(), d.off.data_ptr(), d.n, d.tok.data_ptr(), d.toff.data_ptr())
            got = ctxs[t].sync_count()
            if got != 256 * 48:
                errors.append(f"thread {t}: {got} tokens counted")
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for c in ctxs:
        c.close()
    assert not errors, errors
    info = holds(k, want)
    assert info["table_slots_used"] == 48 and len(k.most_common()) == 48
    k.close()
