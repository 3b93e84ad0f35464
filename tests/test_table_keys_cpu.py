"""tests/table_keys.py keeps its promises, by the reference alone (encode_ref.key_hash, encode_ref.probe), and the host's table builder
(kgpu_vocab_table.cpp, through the kgpu_debug_vocab_table hook) takes what it builds: different words with one full 32-bit hash, and probe chains
that start at the table's last slot and go on at slot 0.  No device.  The stand-alone sanitizer program of the same builder
(tests/c_abi/vocab_table_main.cpp, run by test_encode_cpu.py::test_table_builder_alone_under_asan_ubsan) holds a few of these keys as literals."""
import numpy as np
import pytest

import encode_ref as E
import table_keys as T
from kanpyo_amd import _lib
from golden_cases import synth20k, vocab_table  # noqa: F401  (synth20k: the fixture)


# ---- (a) the builders ----------------------------------------------------------------------------------------------------------------------------
def _is_pair(a, b):
    return isinstance(a, bytes) and isinstance(b, bytes) and a != b and E.key_hash(a) == E.key_hash(b)


def test_fnv_raw_is_the_hash_in_front_of_the_finaliser():
    """Equal fnv_raw <=> equal key_hash on a few thousand short keys, some of which collide by construction (one byte, 256 values, 300 draws)."""
    rng = np.random.default_rng(0)
    for L, n in ((0, 3), (1, 300), (2, 2000), (7, 2000), (33, 500)):
        keys = rng.integers(0, 256, size=(n, L), dtype=np.uint8)
        raw = T.fnv_raw(keys).tolist()
        full = [E.key_hash(k.tobytes()) for k in keys]
        assert len(raw) == n and len(set(raw)) == len(set(full))
        assert len(set(zip(raw, full))) == len(set(raw)), "fnv_raw -> key_hash is one to one"
    assert len(set(T.fnv_raw(np.zeros((4, 1), dtype=np.uint8)).tolist())) == 1
    # a key and the same bytes at another length never share a row: the length is folded in
    assert T.fnv_raw(np.array([[7]], dtype=np.uint8))[0] != T.fnv_raw(np.array([[7, 0]], dtype=np.uint8))[0]


@pytest.mark.parametrize("L, seed", [(5, 1), (8, 2), (21, 3)])
def test_colliding_pairs(L, seed):
    pairs = T.colliding_pairs(L, 12, seed)
    assert len(pairs) == 12 and all(len(a) == len(b) == L and _is_pair(a, b) for a, b in pairs)
    assert len({k for p in pairs for k in p}) == 24, "no key is in two pairs"
    assert all(0 not in k for p in pairs for k in p)
    assert pairs == T.colliding_pairs(L, 12, seed) and pairs[:3] == T.colliding_pairs(L, 3, seed), "deterministic for a seed"
    assert pairs != T.colliding_pairs(L, 12, seed + 100)
    with pytest.raises(ValueError):
        T.colliding_pairs(L, 5, seed, draws=100)


def test_colliding_pairs_behind_a_prefix_and_extended():
    prefix = b"common 16 bytes:"
    (a, b), = T.colliding_pairs(5, 1, 6, prefix=prefix)
    assert _is_pair(a, b) and len(a) == len(b) == 21 and a[:16] == b[:16] == prefix and a[16:] != b[16:]
    base = T.colliding_pairs(5, 1, 1)[0]
    for n in (1, 3, 16, 3067):
        x, y = T.extend(base, T.random_suffix(n, n))
        assert _is_pair(x, y) and len(x) == len(y) == 5 + n and x[5:] == y[5:] and x[:5] == base[0] and y[:5] == base[1]
    assert T.random_suffix(9, 4) == T.random_suffix(9, 4) and 0 not in T.random_suffix(500, 1)
    with pytest.raises(AssertionError):   # a pair of two lengths does not extend: the states in front of the folded length differ
        T.extend(T.cross_length_pairs(8, 7, 1, 4)[0], b"x")
    for slots, home in ((64, 63), (16, 15), (256, 0)):
        x, y = T.pair_with_home(base, slots, home, 4, 3)
        assert _is_pair(x, y) and E.key_hash(x) & (slots - 1) == home and (x, y) == T.pair_with_home(base, slots, home, 4, 3)


def test_cross_length_pairs():
    for La, Lb, seed in ((8, 7, 4), (16, 9, 5)):
        pairs = T.cross_length_pairs(La, Lb, 6, seed)
        assert len(pairs) == 6 and all(len(a) == La and len(b) == Lb and _is_pair(a, b) for a, b in pairs)
        assert pairs == T.cross_length_pairs(La, Lb, 6, seed) and len({k for p in pairs for k in p}) == 12


def test_keys_with_home():
    for slots, home, count in ((64, 61, 120), (16, 15, 40), (64, 0, 10), (256, 253, 40)):
        keys = T.keys_with_home(slots, home, count, 6, 5)
        assert len(keys) == len(set(keys)) == count and all(len(k) == 6 and E.key_hash(k) & (slots - 1) == home for k in keys)
        assert keys == T.keys_with_home(slots, home, count, 6, 5) and keys[:7] == T.keys_with_home(slots, home, 7, 6, 5)
    with pytest.raises(ValueError):
        T.keys_with_home(64, 61, 1000, 6, 5)


def test_lds_home_crowds_every_entry():
    """Every entry of the count kernel's 1024-entry table is the first choice of more rows of the 20 000-record dictionary than the 8 a probe walks."""
    homes = T.lds_home(np.arange(20000)).astype(np.int64)
    per = np.bincount(homes, minlength=T.LDS_ENTRIES)
    assert len(per) == T.LDS_ENTRIES and per.min() >= 12 > T.LDS_PROBES and per.max() <= 21
    assert int(T.lds_home(0)) == 2654435761 >> 22 and int(T.lds_home(1)) == ((2 * 2654435761) & 0xFFFFFFFF) >> 22
    for h in (0, 300, 1023):
        rows = T.rows_with_lds_home(20000, h)
        assert len(rows) == per[h] and all(int(T.lds_home(r)) == h for r in rows)


def test_the_shared_sets():
    same, cross, big = T.adversarial_pairs()
    assert len(same) >= 8 and len(cross) >= 4
    assert all(len(a) == len(b) and _is_pair(a, b) for a, b in same) and all(len(a) != len(b) and _is_pair(a, b) for a, b in cross)
    assert _is_pair(*big) and len(big[0]) == len(big[1]) == 3072 and big[0][8:] == big[1][8:]
    keys = [k for p in same + cross + [big] for k in p]
    assert len(set(keys)) == len(keys) == 2 * (len(same) + len(cross) + 1)
    assert sum(1 for a, _ in same if E.key_hash(a) & 63 == 63) >= 3, "pairs that share home slot 63 of 64"
    assert any(len(a) > 16 and a[8:] == b[8:] for a, b in same), "a pair that differs inside the first arena word only"
    assert any(len(a) > 16 and a[:16] == b[:16] for a, b in same), "a pair that differs in the last arena word only"
    assert T.adversarial_pairs() == (same, cross, big)
    for slots, home, listed in ((16, 15, 8), (64, 63, 32), (64, 61, 48)):
        words, absent, covered = T.chain(slots, home, listed)
        assert len(words) == listed and len(absent) == 4 and len(set(words + absent + covered)) == listed + 4 + listed - 1
        assert all(E.key_hash(k) & (slots - 1) == home for k in words + absent)
        assert [E.key_hash(k) & (slots - 1) for k in covered] == list(range(listed - 1))


def _printable(k):
    return all(0x21 <= c <= 0x7E for c in k)


def test_byte_range_argument():
    """The range bounds every drawn byte, both ends reachable; without it the builders give what they gave (the shared sets above are byte for byte the same)."""
    lo, hi = T.PRINTABLE
    keys = T._draw(np.random.default_rng(1), 5000, 6, b"\x00\xff", T.PRINTABLE)
    assert (keys[:, :2] == [0, 255]).all() and keys[:, 2:].min() == lo == 0x21 and keys[:, 2:].max() == hi == 0x7E
    assert np.array_equal(T._draw(np.random.default_rng(1), 50, 6), T._draw(np.random.default_rng(1), 50, 6, byte_range=T.ANY)) and T.ANY == (1, 255)
    for L, want in ((5, 15), (8, 11)):   # (the counts the draws give: 400 000 keys of 94^L are about 400 000^2 / 2^33 pairs)
        pairs = T.colliding_pairs(L, want, 11 + (L == 8), byte_range=T.PRINTABLE)
        assert len(pairs) == want and all(len(a) == len(b) == L and _is_pair(a, b) and _printable(a + b) for a, b in pairs)
        assert len({k for p in pairs for k in p}) == 2 * want
    pairs = T.cross_length_pairs(8, 7, 30, 13, byte_range=T.PRINTABLE)
    assert len(pairs) == 30 and all(len(a) == 8 and len(b) == 7 and _is_pair(a, b) and _printable(a + b) for a, b in pairs)
    keys = T.keys_with_home(16, 15, 12, 6, 5, byte_range=T.PRINTABLE)
    assert len(set(keys)) == 12 and all(len(k) == 6 and _printable(k) and E.key_hash(k) & 15 == 15 for k in keys)
    assert keys != T.keys_with_home(16, 15, 12, 6, 5)
    words, absent, covered = T.chain(16, 15, 8, byte_range=T.PRINTABLE)
    assert len(set(words + absent + covered)) == 8 + 4 + 7 and all(_printable(k) for k in words + absent + covered)
    assert all(E.key_hash(k) & 15 == 15 for k in words + absent) and [E.key_hash(k) & 15 for k in covered] == list(range(7))
    assert T.chain(16, 15, 8) != (words, absent, covered), "the printable chain is cached beside the 1..255 one, not in its place"


def test_prefix_pairs():
    for L, want in ((7, 4), (6, 2)):
        pairs = T.prefix_pairs(L, want)
        assert len(pairs) == want and len({k for p in pairs for k in p}) == 2 * want
        assert all(len(a) == L + 1 and b == a[:L] and _is_pair(a, b) and _printable(a) for a, b in pairs), "b is a's first L bytes, with a's hash"
        assert pairs == T.prefix_pairs(L, want)


def test_the_wordpiece_pairs():
    same, cross, nested = T.wordpiece_pairs()
    assert len(same) >= 6 and {len(a) for a, _ in same} == {5, 8} and len(cross) >= 4 and len(nested) >= 2
    assert all(len(a) == len(b) and _is_pair(a, b) for a, b in same), "equal hashes, distinct bytes"
    assert all((len(a), len(b)) == (8, 7) and _is_pair(a, b) for a, b in cross + nested)
    assert all(a[:7] != b for a, b in cross) and all(a[:7] == b for a, b in nested)
    keys = [k for p in same + cross + nested for k in p]
    assert len(set(keys)) == len(keys), "no key appears in two pairs"
    assert all(_printable(k) for k in keys), "no byte outside 0x21..0x7E"
    assert T.wordpiece_pairs() == (same, cross, nested)


# ---- (b) the host builder ------------------------------------------------------------------------------------------------------------------------
def _build(synth20k, words, unk_id=-7):
    sd, known, unk, nk, nu, _ = synth20k
    rc, _, slots, arena, _ = vocab_table(sd.dict, known, unk, nk, nu, {}, words, unk_id)
    return rc, slots, arena


def _slot_of(slots, arena, word):
    got, steps = E.probe(slots, arena, word)
    return got, (E.key_hash(word) + steps) & (len(slots) - 1)


def test_builder_keeps_colliding_words_apart(synth20k):
    same, cross, big = T.adversarial_pairs()
    pairs = same + cross + [big]
    assert len(same) >= 8 and len(cross) >= 4 and len(big[0]) == 3072
    vocab = [b"<unk>"] + [k for p in pairs for k in p] + [b"filler-%d" % i for i in range(20)]
    rc, slots, arena = _build(synth20k, vocab)
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    assert len(slots) == 128 and int((slots[:, 0] != 0).sum()) == len(vocab)
    for k, w in enumerate(vocab):
        assert E.probe(slots, arena, w)[0] == k, (k, w[:24])
    for a, b in pairs:
        (ia, sa), (ib, sb) = _slot_of(slots, arena, a), _slot_of(slots, arena, b)
        assert sa != sb and ia != ib and int(slots[sa][0]) >> 32 == int(slots[sb][0]) >> 32 == E.key_hash(a)
    # one key of every pair listed: its partner is absent, whichever of the two it is
    for listed, absent in (([a for a, _ in pairs], [b for _, b in pairs]), ([b for _, b in pairs], [a for a, _ in pairs])):
        rc, slots, arena = _build(synth20k, listed)
        assert rc == _lib.KGPU_OK
        assert [E.probe(slots, arena, w)[0] for w in listed] == list(range(len(listed)))
        for w in absent:
            got, steps = E.probe(slots, arena, w)
            assert got is None and steps >= 1, "the partner's home slot is taken by a word with its hash"
    # the same bytes twice among colliding pairs: still the duplicate error, with both indices
    flat = [k for p in pairs for k in p]
    for first in (0, 1, 2 * len(same) + 1, len(flat) - 1):
        rc, _, _ = _build(synth20k, flat + [flat[first]])
        msg = _lib.lib().kgpu_last_error().decode()
        assert rc == _lib.KGPU_ERR_INVALID_ARG and f" {first} " in msg and f" {len(flat)} " in msg, msg


@pytest.mark.parametrize("slots, listed", [(16, 8), (64, 32)])
def test_builder_wraps_a_chain_around_the_tables_end(synth20k, slots, listed):
    home = slots - 1
    words, absent, covered = T.chain(slots, home, listed)
    assert all(E.key_hash(w) & (slots - 1) == home for w in words + absent) and len(words) == listed
    rc, table, arena = _build(synth20k, words)
    assert rc == _lib.KGPU_OK and len(table) == slots
    assert np.flatnonzero(table[:, 0]).tolist() == list(range(listed - 1)) + [home], "the chain: the last slot, then 0, 1, ..."
    assert [int(table[(home + k) & (slots - 1)][1]) for k in range(listed)] == list(range(listed))
    for k, w in enumerate(words):
        assert E.probe(table, arena, w) == (k, k)
    assert E.probe(table, arena, words[-1])[1] == listed - 1
    for w in absent:   # an absent key of that home walks the whole chain to the free slot behind it
        assert E.probe(table, arena, w) == (None, listed)
    for h, w in enumerate(covered):   # ... and one whose home lies inside the chain walks the rest of it
        assert E.probe(table, arena, w) == (None, listed - 1 - h)
