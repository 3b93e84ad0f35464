"""Text from ids (include/kanpyo_gpu.h, "text from ids"): sequences of vocabulary ids back to the words they stand for, one line per sequence --
`tokenizers.decoders.WordPiece(prefix, cleanup=False)` stated on bytes.  decode_host is the rule on the host (numpy in, numpy out, no device): what
DeviceContext.decode, Vocab.decode_tensor and Vocab.decode compute on the device is defined by it."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._calls import pack_sentences, ptr


def _bytes(w) -> bytes:
    return w.encode("utf-8") if isinstance(w, str) else bytes(w)


def decode_opts(separator=b" ", skip=()) -> "_lib.DecodeOpts":
    """kgpu_decode_opts of a separator (str or bytes, 0..8 bytes) and a skip list (at most 8 ids, any int32); ValueError otherwise."""
    sep = _bytes(separator)
    skip = [int(k) for k in skip]
    if len(sep) > 8:
        raise ValueError(f"the separator {sep!r} has more than 8 bytes")
    if len(skip) > _lib.KGPU_DECODE_MAX_SKIP or any(not -2**31 <= k < 2**31 for k in skip):
        raise ValueError(f"the skip list holds at most {_lib.KGPU_DECODE_MAX_SKIP} ids, each an int32")
    return _lib.DecodeOpts(C.sizeof(_lib.DecodeOpts), 0, len(sep), (C.c_uint8 * 8)(*sep), len(skip), (C.c_int32 * _lib.KGPU_DECODE_MAX_SKIP)(*skip))


def id_sequences(ids, offsets, width: int) -> tuple:
    """The two input forms as the entry points take them -> (ids int32, offsets uint64 or None, n, width).  offsets given: ragged (width 0).
    offsets None: padded -- a 2-D ids gives its own width, a flat one is cut into rows of `width`."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.size < 1 or width:
            raise ValueError("ragged: offsets has n + 1 entries and width is 0")
        return ids.reshape(-1), offsets, offsets.size - 1, 0
    if ids.ndim == 2:
        width = width or ids.shape[1]
        if width != ids.shape[1]:
            raise ValueError("padded: width is the rows' length")
        n = ids.shape[0] if width else 0
    else:
        if width < 1 or ids.size % width:
            raise ValueError("padded: width is 1 or more and divides the ids")
        n = ids.size // width
    if width < 1:
        raise ValueError("padded: width is 1 or more")
    return ids.reshape(-1), None, n, int(width)


def host_call(entry, ids, offsets, width, opts, text_capacity=None) -> tuple:
    """entry(ids_ptr, offsets_ptr, n, width, opts, text_ptr, capacity, text_offsets_ptr, status_ptr, byref(got)) -> rc, over the two input forms:
    kgpu_decode_host and kgpu_decode_batch behind their leading arguments.  -> (text uint8, text_offsets uint64 [n + 1], status uint8 [n]).
    text_capacity None: one more call with the size the library reports; a number: that many bytes, and KgpuError with KGPU_ERR_CAPACITY
    (err.bytes: the size needed) when it is too small."""
    ids, offsets, n, width = id_sequences(ids, offsets, width)
    toff, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
    got = C.c_uint64(0)
    cap = ids.size * 8 + 64 if text_capacity is None else int(text_capacity)
    while True:
        text = np.empty(max(cap, 1), dtype=np.uint8)
        rc = entry(ptr(ids), None if offsets is None else offsets.ctypes.data, n, width, C.byref(opts) if opts is not None else None, text.ctypes.data, cap,
                   toff.ctypes.data, status.ctypes.data, C.byref(got))
        if rc == _lib.KGPU_ERR_CAPACITY and text_capacity is None and int(got.value) > cap:
            cap = int(got.value)
            continue
        if rc != _lib.KGPU_OK:
            err = _lib.KgpuError(rc, _lib.lib().kgpu_last_error().decode("utf-8", "replace"))
            err.bytes = int(got.value)
            raise err
        return text[: int(got.value)], toff, status[:n]


def decode_host(words: Sequence, ids, offsets=None, width: int = 0, prefix=b"", separator=b" ", skip=(), text_capacity=None) -> tuple:
    """kgpu_decode_host: the list `words` (str or bytes; id k is words[k]), ragged ids (ids int32 with offsets uint64 [n + 1]) or padded ones (offsets
    None: a 2-D ids, or a flat one with its width); prefix: the WordPiece continuation prefix (at most 8 bytes; empty: a plain vocabulary).
    -> (text uint8, text_offsets uint64 [n + 1], status uint8 [n]): line s is text[text_offsets[s]:text_offsets[s + 1]]; status 1: an id outside
    the list that the skip list does not name."""
    from functools import partial

    wp, woff = pack_sentences([_bytes(w) for w in words])
    wp = np.ascontiguousarray(wp)
    pre = np.frombuffer(_bytes(prefix), dtype=np.uint8)
    entry = partial(_lib.lib().kgpu_decode_host, ptr(wp), woff.ctypes.data, woff.size - 1, ptr(pre), pre.size)
    return host_call(entry, ids, offsets, width, decode_opts(separator, skip), text_capacity)


def lines(text: np.ndarray, text_offsets: np.ndarray) -> list:
    """(text, text_offsets) -> one bytes object per line."""
    raw, o = np.asarray(text, dtype=np.uint8).tobytes(), np.asarray(text_offsets).tolist()
    return [raw[o[i] : o[i + 1]] for i in range(len(o) - 1)]
