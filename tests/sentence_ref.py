"""The sentence rule (include/kanpyo_gpu.h, "sentences") restated in plain Python with an explicit bracket stack -- not the scan form the library
runs.  Works on bytes: a class is the occurrence of a code point's complete UTF-8 encoding inside the line, on invalid text too."""
import ctypes as C

import numpy as np

DEFAULT_TERMINATORS = "。｡！？!?"
OPENERS = "「『（(［[｛{〈《【〔｢"
CLOSERS = "」』）)］]｝}〉》】〕｣"
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
SPACES = "".join(chr(c) for c in WHITE_SPACE)

SENTENCE_DTYPE = np.dtype([("line", "<u8"), ("byte_start", "<u4"), ("char_start", "<u4")])


def _encodings(chars):
    return [c.encode("utf-8") for c in chars]


def _match(line: bytes, i: int, encs):
    """Length of the encoding of `encs` that starts at line[i], or 0."""
    for e in encs:
        if line.startswith(e, i):
            return len(e)
    return 0


def split_line(line: bytes, terminators=None, brackets=True):
    """-> [(byte_start, byte_end)] of the line's sentences."""
    terms = _encodings(terminators if terminators else DEFAULT_TERMINATORS)
    opens, closes, spaces = _encodings(OPENERS), _encodings(CLOSERS), _encodings(SPACES)
    n = len(line)
    # enclosing depth: the matched pairs (o, c) with o <= j < c
    eff = [0] * (n + 1)
    if brackets:
        stack, pairs = [], []
        for i in range(n):
            if _match(line, i, opens):
                stack.append(i)
            elif _match(line, i, closes) and stack:
                pairs.append((stack.pop(), i))
        for o, c in pairs:   # +1 over [o, c): as differences, then summed
            eff[o] += 1
            eff[c] -= 1
        for j in range(1, n + 1):
            eff[j] += eff[j - 1]
    cuts = []   # (end of the sentence in front, start of the next)
    i = 0
    while i < n:
        tl = _match(line, i, terms)
        if not tl:
            i += 1
            continue
        e = i + tl
        if not _match(line, e, terms) and eff[i] == 0:
            p = e
            while p < n:
                sl = _match(line, p, spaces)
                if not sl:
                    break
                p += sl
            if p < n:
                cuts.append((e, p))
        i = e
    out, b = [], 0
    for e, p in cuts:
        out.append((b, e))
        b = p
    out.append((b, n))
    return out


def split_lines(lines, terminators=None, brackets=True):
    """lines: list of bytes -> (text bytes, offsets list, records list of (line, byte_start, char_start))."""
    text, offs, recs = bytearray(), [0], []
    for li, line in enumerate(lines):
        for b, e in split_line(line, terminators, brackets):
            text += line[b:e]
            offs.append(len(text))
            recs.append((li, b, sum(1 for x in line[:b] if x & 0xC0 != 0x80)))
    return bytes(text), offs, recs


def pack(lines):
    """list of bytes -> (utf8 uint8 array, offsets uint64 array)"""
    offs = np.zeros(len(lines) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in lines], dtype=np.uint64) if lines else []
    return np.frombuffer(b"".join(lines), np.uint8).copy(), offs


class SentenceOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("n_terminators", C.c_uint32), ("terminators", C.c_uint32 * 16), ("reserved", C.c_uint32 * 2)]


def make_opts(terminators=None, brackets=True):
    o = SentenceOpts()
    o.flags = 0 if brackets else 1
    cps = [ord(c) for c in terminators] if terminators else []
    o.n_terminators = len(cps)
    for k, c in enumerate(cps[:16]):
        o.terminators[k] = c
    return o
