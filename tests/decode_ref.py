"""Rules 1 to 3 of include/kanpyo_gpu.h, "text from ids", restated on Python bytes: the reference the CPU and GPU decode tests compare with.
Nothing of the library is used here."""
import random

OK, BAD_ID = 0, 1
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def decode_one(words, ids, prefix=b"", sep=b" ", skip=()):
    """One sequence -> (its line, its status byte)."""
    out, kept, status = [], 0, OK
    for i in ids:
        if i in skip:                       # rule 1: the skip list first, whatever the id's range
            continue
        if not 0 <= i < len(words):
            status = BAD_ID
            continue
        w = words[i]
        if kept == 0:                       # rule 2: kept element 0 as it is
            out.append(w)
        elif prefix and w.startswith(prefix):
            out.append(w[len(prefix):])     # the prefix goes, once
        else:
            out.append(sep + w)
        kept += 1
    return b"".join(out), status


def decode(words, sequences, prefix=b"", sep=b" ", skip=()):
    """-> (lines, status bytes)."""
    got = [decode_one(words, s, prefix, sep, skip) for s in sequences]
    return [g[0] for g in got], [g[1] for g in got]


def sequences_of(ids, offsets=None, width=0):
    """The two input forms -> a list of id lists."""
    ids = [int(x) for x in ids]
    if offsets is not None:
        o = [int(x) for x in offsets]
        return [ids[o[s]:o[s + 1]] for s in range(len(o) - 1)]
    return [ids[s * width:(s + 1) * width] for s in range(len(ids) // width)] if width else []


WORD_LENGTHS = (1, 7, 8, 9, 64, 65, 3072)


def random_list(rng: random.Random, prefix: bytes, n_words: int):
    """A list of n_words DISTINCT entries that holds (as far as n_words allows) the empty word, a word equal to the prefix, a doubled-prefix word, words of
    the lengths at which a load or a unit changes, and words that are not UTF-8."""
    special = [b"", prefix, prefix + prefix + b"y", prefix + b"ab", b"\xff\xfe", b"\x80", prefix + b"\xc3"]
    special += [rng.randbytes(n) for n in WORD_LENGTHS]
    special += [prefix + bytes(rng.randrange(97, 123) for _ in range(n)) for n in (1, 8, 64)]
    rng.shuffle(special)
    seen, out = set(), []
    for w in special:
        if w not in seen and len(out) < n_words:
            seen.add(w)
            out.append(w)
    while len(out) < n_words:
        w = bytes(rng.randrange(97, 123) for _ in range(rng.randrange(1, 12)))
        if rng.random() < 0.3:
            w = prefix + w
        if w not in seen:
            seen.add(w)
            out.append(w)
    rng.shuffle(out)
    return out


def random_case(rng: random.Random):
    """One seeded case of the CPU sweep -> dict(words, prefix, sep, skip, ids, offsets or None, width)."""
    prefix = rng.choice((b"", b"##", b"@@cont@@"))                       # prefix lengths 0, 2, 8
    sep = rng.choice((b"", b" ", b"\xe3\x80\x80", b"<--sep->"))          # separators of 0, 1, 3, 8 bytes
    words = random_list(rng, prefix, rng.choice((1, 2, 3, 17, 40, 200)) if rng.random() < 0.5 else rng.randrange(1, 201))
    nw = len(words)
    odd = [-1, nw, INT32_MIN, INT32_MAX, nw + 7]
    n_skip = rng.choice((0, 1, 8))
    pool = sorted(set(range(min(nw, 12))) | set(odd))                    # ids inside the list and outside it
    skip = rng.sample(pool, min(n_skip, len(pool)))
    n = rng.choice((0, 1, 2, 5, 9))

    def one_id():
        r = rng.random()
        if r < 0.12:
            return rng.choice(odd)
        if r < 0.3 and skip:
            return rng.choice(skip)
        return rng.randrange(nw)

    if rng.random() < 0.5:   # ragged; a few leading ids nobody owns, empty sequences among the rest
        lens = [rng.choice((0, 0, 1, 2, 3, 8, 20)) for _ in range(n)]
        lead = rng.randrange(3)
        offsets = [lead]
        for ln in lens:
            offsets.append(offsets[-1] + ln)
        ids = [one_id() for _ in range(offsets[-1] + rng.randrange(2))]
        return dict(words=words, prefix=prefix, sep=sep, skip=skip, ids=ids, offsets=offsets, width=0)
    width = rng.choice((1, 2, 7, 16))
    return dict(words=words, prefix=prefix, sep=sep, skip=skip, ids=[one_id() for _ in range(n * width)], offsets=None, width=width)
