"""User dictionary (include/kanpyo_gpu.h, "user dictionary"): extra words beside the uploaded dictionary -- product names, new coinages, a customer's
own vocabulary -- matched against the text and laid beside the lattice on the device.  UserDict is the handle (a few kilobytes: many may live over one
Tokenizer); userdict_host is the rule on the host (a Lattice and its sentence in, numpy out, no device): what Tokenizer.tokenize_user_packed computes
on the device is defined by it."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Sequence

import numpy as np

from . import _lib
from ._calls import TOKEN_DTYPE, Handle, grown, ptr, struct_dict
from .nbest import connection_matrix, lattice_struct


class UserEntry(NamedTuple):
    """One line of a MeCab user CSV: surface,left_id,right_id,cost,feature,..."""

    surface: str
    left_id: int
    right_id: int
    cost: int
    features: tuple = ()


class UserDictFormatError(ValueError):
    """A CSV line that is no entry; `line` is its 1-based number."""

    def __init__(self, line: int, why: str):
        super().__init__(f"user dictionary line {line}: {why}")
        self.line = line


def parse_csv(text: str, normalize=None) -> list:
    """MeCab's user dictionary format, one entry per line: surface,left_id,right_id,cost,feature,... -> [UserEntry].  Empty lines and lines that start
    with '#' are skipped.  A field may be quoted with '"' ('""' inside: a quote), so that a surface can hold a comma.  normalize="NFC" / "NFKC": the
    surfaces go through normalize_host in that form -- a half-width key can otherwise never match normalised text.  UserDictFormatError names a bad line."""
    import csv

    out = []
    for no, line in enumerate(text.split("\n"), 1):   # ('\n' alone ends a line: a surface may hold U+0085, U+2028 and their like)
        line = line[:-1] if line.endswith("\r") else line
        if not line.strip() or line.startswith("#"):
            continue
        try:
            fields = next(csv.reader([line]))
        except (csv.Error, StopIteration) as e:
            raise UserDictFormatError(no, f"not CSV ({e})") from None
        if len(fields) < 4:
            raise UserDictFormatError(no, "fewer than four fields (surface,left_id,right_id,cost,feature,...)")
        if not fields[0]:
            raise UserDictFormatError(no, "an empty surface")
        try:
            left, right, cost = (int(f.strip()) for f in fields[1:4])
        except ValueError:
            raise UserDictFormatError(no, "left_id, right_id and cost are integers") from None
        if not (0 <= left <= 0xFFFF and 0 <= right <= 0xFFFF and -0x8000 <= cost <= 0x7FFF):
            raise UserDictFormatError(no, "a context id outside 0..65535 or a cost outside an int16")
        surface = fields[0]
        if normalize is not None:
            from .tokenizer import normalize_host

            surface = normalize_host(surface, normalize).decode("utf-8")
        out.append(UserEntry(surface, left, right, cost, tuple(fields[4:])))
    return out


def _entry_arrays(entries: Sequence) -> tuple:
    """[UserEntry or (surface, left_id, right_id, cost, ...)] -> (keys[uint8], key_offsets[uint64 E+1], left[uint16], right[uint16], cost[int16])."""
    enc = [e[0].encode("utf-8") if isinstance(e[0], str) else bytes(e[0]) for e in entries]
    koff = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        koff[1:] = np.cumsum(np.fromiter((len(k) for k in enc), dtype=np.uint64, count=len(enc)))
    for e in entries:
        if not (0 <= int(e[1]) <= 0xFFFF and 0 <= int(e[2]) <= 0xFFFF and -0x8000 <= int(e[3]) <= 0x7FFF):
            raise ValueError(f"user dictionary entry {e[0]!r}: a context id outside 0..65535 or a cost outside an int16")
    return (np.frombuffer(b"".join(enc), dtype=np.uint8), koff, np.array([int(e[1]) for e in entries], dtype=np.uint16),
            np.array([int(e[2]) for e in entries], dtype=np.uint16), np.array([int(e[3]) for e in entries], dtype=np.int16))


def _entry_args(arrays: tuple) -> tuple:
    keys, koff, left, right, cost = arrays
    return ptr(keys), koff.ctypes.data, ptr(left), ptr(right), ptr(cost), koff.size - 1


class UserDict(Handle):
    """kgpu_userdict: entries over one Tokenizer's dictionary.  entries: UserEntry objects, or tuples (surface, left_id, right_id, cost[, features]).
    The context ids are the dictionary's own; several entries may share a surface.  Destroy it (close()) before the tokenizer.  A token of class
    TokenClass.User carries id = the entry's index + 1: features(id) gives the entry's feature list, entry(id) the entry."""

    _destroy = "kgpu_userdict_destroy"

    def __init__(self, tokenizer, entries: Sequence = ()):
        self.tokenizer = tokenizer
        self.entries = [e if isinstance(e, UserEntry) else UserEntry(e[0], int(e[1]), int(e[2]), int(e[3]), tuple(e[4]) if len(e) > 4 else ()) for e in entries]
        arrays = _entry_arrays(self.entries)
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_userdict_create(tokenizer.handle, *_entry_args(arrays), C.byref(h)))
        self._h = h

    @classmethod
    def from_csv(cls, tokenizer, text_or_path, normalize=None) -> "UserDict":
        """A MeCab user CSV (parse_csv), given as the path of a file (UTF-8) -- an os.PathLike, or a str that names an existing file -- or as its text."""
        text = text_or_path
        if isinstance(text_or_path, os.PathLike) or (isinstance(text_or_path, str) and "\n" not in text_or_path and os.path.exists(text_or_path)):
            with open(text_or_path, encoding="utf-8", newline="") as f:
                text = f.read()
        return cls(tokenizer, parse_csv(text, normalize))

    def __len__(self) -> int:
        return len(self.entries)

    def entry(self, token_id: int) -> UserEntry:
        return self.entries[int(token_id) - 1]

    def features(self, token_id: int) -> list:
        return list(self.entries[int(token_id) - 1].features)

    def info(self) -> dict:
        i = _lib.UserdictInfo()
        _lib.check(_lib.lib().kgpu_userdict_get_info(self._h, C.byref(i)))
        return struct_dict(i)


def invoke_bytes(dict, text) -> np.ndarray:
    """One byte per character of text: 1 where the character's category is in the Dict's invoke_list (char_category_def.rs:33-38: a code point beyond the
    table has the category of code point 0)."""
    s = text if isinstance(text, str) else bytes(text).decode("utf-8")
    cat, inv = dict.char_category, dict.invoke_list
    out = np.zeros(max(len(s), 1), dtype=np.uint8)
    for i, ch in enumerate(s):
        c = int(cat[ord(ch)] if ord(ch) < cat.size else cat[0])
        out[i] = 1 if c < inv.size and inv[c] else 0
    return out[: len(s)]


def userdict_host(lattice, text, connection, dict, entries: Sequence, mode="normal", penalties=None) -> tuple:
    """kgpu_userdict_host -> (tokens[TOKEN_DTYPE], cost): the records of the best path over the lattice widened by the entries' matches, and dp of EOS.
    text: the lattice's sentence (str or bytes); connection: see nbest.connection_matrix; dict: the Dict whose char_category and invoke_list tell which
    positions keep their unknown words (or the invoke bytes themselves, one per character); entries as UserDict takes them.  Needs no device."""
    from .mode import mode_opts

    lat, keep = lattice_struct(lattice)
    conn, rows, cols = connection_matrix(connection)
    raw = np.frombuffer(text.encode("utf-8") if isinstance(text, str) else bytes(text), dtype=np.uint8)
    if isinstance(dict, (bytes, bytearray)):
        invoke = np.frombuffer(bytes(dict), dtype=np.uint8)
    else:
        invoke = np.ascontiguousarray(dict, dtype=np.uint8) if isinstance(dict, (np.ndarray, list, tuple)) else invoke_bytes(dict, raw.tobytes())
    arrays = _entry_arrays(entries)
    opts = mode if isinstance(mode, _lib.ModeOpts) else mode_opts(mode, penalties)
    caps = (len(lattice.nodes),)   # (grown to the exact size where extended mode gives more records than the lattice has nodes)
    T, cost = C.c_uint64(0), C.c_int32(0)
    while caps is not None:
        tokens = np.zeros(max(caps[0], 1), dtype=TOKEN_DTYPE)
        rc = _lib.lib().kgpu_userdict_host(C.byref(lat), ptr(raw), raw.size, conn.ctypes.data, rows, cols, ptr(invoke), *_entry_args(arrays), C.byref(opts),
                                           tokens.ctypes.data, caps[0], C.byref(T), C.byref(cost))
        caps = grown(rc, caps, (T.value,))
    del keep
    return tokens[: T.value], cost.value
