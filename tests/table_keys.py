"""Adversarial keys for the byte-keyed tables of the word counts, the vocabulary ids and the WordPiece ids (kgpu_count.hip, kgpu_encode.hip,
kgpu_wordpiece.hip, kgpu_vocab_table.cpp): different byte strings with one full 32-bit hash -- of one length, of two, and a key with the hash of its own
first bytes --, keys with a chosen home slot, feature rows with a chosen entry of the count kernel's LDS table.  A byte range (PRINTABLE) keeps keys to
one-byte characters for the WordPiece matcher, which probes a word at every character end.

Input construction only, on numpy and Python bytes; nothing comes from the library and NO EXPECTED VALUE COMES FROM HERE: what a test expects is
count_ref's / encode_ref's answer on the crafted records.  The table's hash is encode_ref.key_hash, the only restatement of it; fnv_raw below is
the part of it in front of murmur3's finaliser, vectorised.  The finaliser is a bijection on 32 bits, so equal fnv_raw means an equal key_hash --
tests/test_table_keys_cpu.py asserts every promise made here by encode_ref.key_hash alone."""
import numpy as np

import encode_ref as E

DRAWS = 400_000   # random keys per search: n^2 / 2^33 = 18.6 expected pairs of one length, n^2 / 2^32 = 37 of two lengths


def fnv_raw(keys):
    """FNV-1a over every row of a uint8 [n, L] array, the length folded in -> uint32 [n]: key_hash before the finaliser."""
    keys = np.asarray(keys, dtype=np.uint8)
    assert keys.ndim == 2
    h = np.full(keys.shape[0], 2166136261, dtype=np.uint64)
    for j in range(keys.shape[1]):
        h = ((h ^ keys[:, j]) * np.uint64(16777619)) & np.uint64(0xFFFFFFFF)
    return (h ^ np.uint64(keys.shape[1] & 0xFFFFFFFF)).astype(np.uint32)


ANY, PRINTABLE = (1, 255), (0x21, 0x7E)   # byte ranges, both ends included.  PRINTABLE: one-byte characters, so every byte boundary is a character end


def _draw(rng, n, L, prefix=b"", byte_range=ANY):
    keys = np.empty((n, len(prefix) + L), dtype=np.uint8)
    keys[:, : len(prefix)] = np.frombuffer(prefix, dtype=np.uint8)
    keys[:, len(prefix) :] = rng.integers(byte_range[0], byte_range[1] + 1, size=(n, L), dtype=np.uint8)
    return keys


def colliding_pairs(L, want, seed, prefix=b"", draws=DRAWS, byte_range=ANY):
    """`want` pairs (a, b) of DIFFERENT byte strings of len(prefix) + L bytes each with one hash: `draws` keys of the prefix and L random bytes 1..255 (or of
    byte_range) from the seed, sorted by fnv_raw, equal neighbours taken in that order.  No key is in two pairs.  A prefix leaves the pair differing in its
    LAST L bytes only."""
    keys = _draw(np.random.default_rng(seed), draws, L, prefix, byte_range)
    h = fnv_raw(keys)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    out, last = [], -1
    for k in np.flatnonzero(hs[1:] == hs[:-1]).tolist():
        a, b = keys[order[k]].tobytes(), keys[order[k + 1]].tobytes()
        if k > last and a != b:
            out.append((a, b))
            last = k + 1
            if len(out) == want:
                return out
    raise ValueError(f"{draws} keys of {L} bytes, seed {seed}: {len(out)} colliding pairs, {want} wanted")


def cross_length_pairs(La, Lb, want, seed, draws=DRAWS, byte_range=ANY):
    """`want` pairs (a, b) with len(a) == La != Lb == len(b) and one hash: `draws` random keys of each length, bytes 1..255 (or of byte_range), from the seed."""
    assert La != Lb
    rng = np.random.default_rng(seed)
    ka, kb = _draw(rng, draws, La, byte_range=byte_range), _draw(rng, draws, Lb, byte_range=byte_range)
    _, ia, ib = np.intersect1d(fnv_raw(ka), fnv_raw(kb), return_indices=True)
    if len(ia) < want:
        raise ValueError(f"{draws} keys of {La} and of {Lb} bytes, seed {seed}: {len(ia)} colliding pairs, {want} wanted")
    return [(ka[i].tobytes(), kb[j].tobytes()) for i, j in zip(ia[:want].tolist(), ib[:want].tolist())]


def extend(pair, suffix):
    """Suffix extension: FNV-1a's state is its running hash, so a + s and b + s collide for every s whenever a and b collide AT EQUAL LENGTH."""
    a, b = pair
    assert len(a) == len(b) and a != b
    return a + bytes(suffix), b + bytes(suffix)


def random_suffix(n, seed):
    return np.random.default_rng(seed).integers(1, 256, size=n, dtype=np.uint8).tobytes()


def pair_with_home(pair, slots, home, suffix_len, seed, tries=100_000):
    """The pair extended by the first random suffix of suffix_len bytes (from the seed) that puts both keys on home slot `home` of `slots`."""
    assert slots & (slots - 1) == 0 and 0 <= home < slots
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        s = rng.integers(1, 256, size=suffix_len, dtype=np.uint8).tobytes()
        if E.key_hash(pair[0] + s) & (slots - 1) == home:
            return extend(pair, s)
    raise ValueError(f"no suffix of {suffix_len} bytes in {tries} puts the pair on slot {home} of {slots}")


def keys_with_home(slots, home, count, length, seed, draws=20_000, byte_range=ANY):
    """`count` distinct keys of `length` random bytes 1..255 (or of byte_range; from the seed, in the order drawn) whose key_hash & (slots - 1) == home."""
    assert slots & (slots - 1) == 0 and 0 <= home < slots
    keys = _draw(np.random.default_rng(seed), draws, length, byte_range=byte_range)
    out, seen = [], set()
    for row in keys:
        k = row.tobytes()
        if k not in seen and E.key_hash(k) & (slots - 1) == home:
            seen.add(k)
            out.append(k)
            if len(out) == count:
                return out
    raise ValueError(f"{draws} keys of {length} bytes, seed {seed}: {len(out)} with home {home} of {slots}, {count} wanted")


FNV_PRIME = 16777619
FNV_PRIME_INV = pow(FNV_PRIME, -1, 1 << 32)


def prefix_pairs(L, want, byte_range=PRINTABLE):
    """`want` pairs (a, b) with one hash where b IS a's first L bytes and len(a) == L + 1: a probe of b meets an entry that starts with the very bytes probed
    and is one byte longer.  Random draws never give one (b is chosen by a), so the pair is solved for: with t = (state after b) ^ (a's last byte x), the
    hashes agree when t * P == t ^ x ^ L ^ (L + 1) mod 2^32, which is solved bit by bit from the low end (P is odd: the low k bits of t decide the low k bits
    of both sides); the L bytes of b that reach that state from FNV's offset basis are found by meeting in the middle, 3 bytes forward, 3 backward
    (a step is undone by P's inverse) behind every choice of b's last L - 6 bytes.  Deterministic; no key is in two pairs."""
    import itertools

    assert L >= 6
    alphabet = np.arange(byte_range[0], byte_range[1] + 1, dtype=np.uint64)
    n, M = len(alphabet), np.uint64(0xFFFFFFFF)

    def digits(i):   # entry i of a three-byte sweep spells three alphabet digits, the first byte swept first
        return [(i // n ** (2 - j)) % n for j in range(3)]

    fwd = np.array([2166136261], dtype=np.uint64)
    for _ in range(3):   # the states after b's first 3 bytes
        fwd = (((fwd[:, None] ^ alphabet[None, :]) * np.uint64(FNV_PRIME)) & M).reshape(-1)
    out, seen = [], set()
    for x in alphabet.tolist():
        c, sols = x ^ L ^ (L + 1), [0]
        for k in range(32):
            mask = (1 << (k + 1)) - 1
            sols = [t | (bit << k) for t in sols for bit in (0, 1) if (((t | (bit << k)) * FNV_PRIME) ^ (t | (bit << k)) ^ c) & mask == 0]
        for t in sols:   # t ^ x: the state b must reach.  b's last L - 6 bytes one by one, the 3 in front of them swept (last byte first), then the meeting
            for last in itertools.product(alphabet.tolist(), repeat=L - 6):
                state = t ^ x
                for y in last[::-1]:
                    state = ((state * FNV_PRIME_INV) & 0xFFFFFFFF) ^ y
                back = np.array([state], dtype=np.uint64)
                for _ in range(3):
                    back = (((back * np.uint64(FNV_PRIME_INV)) & M)[:, None] ^ alphabet[None, :]).reshape(-1)
                _, i_f, i_b = np.intersect1d(fwd, back, return_indices=True)
                for f, r in zip(i_f.tolist(), i_b.tolist()):
                    b = bytes(int(alphabet[d]) for d in digits(f) + digits(r)[::-1]) + bytes(last)
                    a = b + bytes([x])
                    if a not in seen and b not in seen:
                        seen |= {a, b}
                        out.append((a, b))
                        if len(out) == want:
                            return out
    raise ValueError(f"{len(out)} pairs of {L + 1} bytes and their first {L}, {want} wanted")


LDS_ENTRIES, LDS_PROBES = 1024, 8


def lds_home(row):
    """The first entry the count kernel's workgroup table tries for feature row `row` (an int or an array): ((row + 1) * 2654435761 mod 2^32) >> 22.
    This mirrors lds_add of kgpu_count.hip -- LH = 1024 entries (LDS_ENTRIES), LDS_PROBES = 8 steps, then a direct add to the row's dense counter --
    ONLY TO CHOOSE INPUTS that crowd that table.  No expected value comes from it: were it out of step with the kernel, the tests that use it would
    still expect the right counts and merely crowd the table less."""
    return ((np.asarray(row, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


def rows_with_lds_home(n_rows, home):
    """The rows 0..n_rows - 1 whose lds_home is `home`, ascending."""
    return np.flatnonzero(lds_home(np.arange(n_rows)) == home).tolist()


# ---- the sets the CPU and GPU tests share (every property is asserted by tests/test_table_keys_cpu.py from encode_ref.key_hash alone) ---------------
_CACHE = {}


def adversarial_pairs():
    """-> (same, cross, big): lists of colliding pairs (a, b), all keys distinct.
    same   ten pairs of equal length: 5, 8 and 21 random bytes; one that differs only in its LAST 5 bytes of 21 (behind a common 16-byte prefix); one
           that differs only in its FIRST 5 bytes of 21, inside the first 8-byte word of an arena entry (suffix extension); three extended by
           suffixes that put all six keys on home slot 63 of a 64-slot table
    cross  six pairs of unequal length: 8 against 7 bytes, 16 against 9
    big    one pair of 3072 bytes that differs in its first 8 bytes only"""
    if "pairs" not in _CACHE:
        p5, p8 = colliding_pairs(5, 8, 1), colliding_pairs(8, 3, 2)
        same = p5[:2] + p8[:2] + colliding_pairs(21, 1, 3) + colliding_pairs(5, 1, 6, prefix=b"common 16 bytes:")
        same.append(extend(p5[2], random_suffix(16, 7)))
        same += [pair_with_home(p, 64, 63, 3 + k, 8 + k) for k, p in enumerate(p5[3:6])]
        cross = cross_length_pairs(8, 7, 4, 4) + cross_length_pairs(16, 9, 2, 5)
        big = extend(p8[2], random_suffix(3064, 9))
        _CACHE["pairs"] = (same, cross, big)
    same, cross, big = _CACHE["pairs"]
    return list(same), list(cross), big


def wordpiece_pairs():
    """-> (same, cross, nested): colliding pairs (a, b) of printable bytes 0x21..0x7E -- one-byte characters, so a WordPiece matcher probes every one of
    their prefixes --, all keys distinct.
    same    eight pairs of equal length: four of 5 bytes, four of 8
    cross   four pairs of 8 against 7 bytes (random draws: the 7 bytes are not the 8-byte key's first)
    nested  two pairs of 8 against 7 bytes where b IS a's first 7 bytes (prefix_pairs)"""
    if "wordpiece" not in _CACHE:
        same = colliding_pairs(5, 4, 11, byte_range=PRINTABLE) + colliding_pairs(8, 4, 12, byte_range=PRINTABLE)
        _CACHE["wordpiece"] = (same, cross_length_pairs(8, 7, 4, 13, byte_range=PRINTABLE), prefix_pairs(7, 2))
    return tuple(list(x) for x in _CACHE["wordpiece"])


def chain(slots, home, listed, absent=4, length=6, seed=5, byte_range=ANY):
    """-> (words, absent_home, absent_covered): `listed` keys of home slot `home` of `slots` -- inserted in this order they occupy home, home + 1, ...
    around the table's end --, `absent` further keys of that home, and one key of every home slot 0..listed - 2 (slots the chain covers when it starts at
    the table's last slot)."""
    key = ("chain", slots, home, listed, absent, length, seed) + ((byte_range,) if byte_range != ANY else ())
    if key not in _CACHE:
        ks = keys_with_home(slots, home, listed + absent, length, seed, byte_range=byte_range)
        covered = [keys_with_home(slots, h, 1, length, seed + 1 + h, byte_range=byte_range)[0] for h in range(listed - 1)]
        _CACHE[key] = (ks[:listed], ks[listed:], covered)
    return tuple(list(x) for x in _CACHE[key])
