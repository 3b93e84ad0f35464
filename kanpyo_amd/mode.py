"""Search and extended modes (include/kanpyo_gpu.h, "search mode"): one-best with a length penalty on long words, so that a compound gives way to its
parts where the dictionary has them; extended mode also cuts unknown words into characters.  mode_host is the rule on the host (a Lattice and its
sentence in, numpy out, no device): what Tokenizer.tokenize_mode_packed computes on the device is defined by it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._calls import TOKEN_DTYPE, grown
from .nbest import connection_matrix, lattice_struct

MODES = {"normal": _lib.KGPU_MODE_NORMAL, "search": _lib.KGPU_MODE_SEARCH, "extended": _lib.KGPU_MODE_EXTENDED}
PENALTIES_DEFAULT = (2, 3000, 7, 1700)   # kanji_length, kanji_penalty, other_length, other_penalty: KGPU_MODE_OPTS_DEFAULT


def mode_opts(mode="search", penalties=None) -> "_lib.ModeOpts":
    """"normal" / "search" / "extended" (any case) or the header's 0 / 1 / 2, and (kanji_length, kanji_penalty, other_length, other_penalty) or None
    for the defaults -> kgpu_mode_opts.  ValueError for a name or a tuple that is none of these; a number out of range is the library's to refuse."""
    key = mode.lower() if isinstance(mode, str) else mode
    if isinstance(key, str):
        if key not in MODES:
            raise ValueError(f"unknown mode {mode!r}: normal, search or extended")
        key = MODES[key]
    pen = PENALTIES_DEFAULT if penalties is None else tuple(int(v) for v in penalties)
    if len(pen) != 4 or any(v < 0 or v > 0xFFFFFFFF for v in pen):
        raise ValueError("penalties: (kanji_length, kanji_penalty, other_length, other_penalty), each an unsigned 32-bit number")
    return _lib.ModeOpts(int(key), *pen, (C.c_uint32 * 3)(0, 0, 0))


def mode_host(lattice, text, connection, mode="search", penalties=None) -> tuple:
    """kgpu_mode_host -> (tokens[TOKEN_DTYPE], cost): the records of the lattice's best path under the mode's penalised costs and dp of EOS (1 << 30
    where nothing was accepted).  text: the lattice's sentence (str or bytes); connection: see nbest.connection_matrix.  Needs no device."""
    lat, keep = lattice_struct(lattice)
    conn, rows, cols = connection_matrix(connection)
    raw = np.frombuffer(text.encode("utf-8") if isinstance(text, str) else bytes(text), dtype=np.uint8)
    opts = mode if isinstance(mode, _lib.ModeOpts) else mode_opts(mode, penalties)
    caps = (len(lattice.nodes),)   # (grown to the exact size where extended mode gives more records than the lattice has nodes)
    T, cost = C.c_uint64(0), C.c_int32(0)
    while caps is not None:
        tokens = np.zeros(max(caps[0], 1), dtype=TOKEN_DTYPE)
        rc = _lib.lib().kgpu_mode_host(C.byref(lat), raw.ctypes.data if raw.size else None, raw.size, conn.ctypes.data, rows, cols, C.byref(opts),
                                       tokens.ctypes.data, caps[0], C.byref(T), C.byref(cost))
        caps = grown(rc, caps, (T.value,))
    del keep
    return tokens[: T.value], cost.value
