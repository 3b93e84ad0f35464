"""The call protocols of the host entry points (include/kanpyo_gpu.h), each written once: the packed input, the result arrays, the one more
call with the size the library reports, and the life of a handle.  Needs ctypes, numpy and _lib only; nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Sequence

import numpy as np

from . import _lib

# kgpu_token (include/kanpyo_gpu.h)
TOKEN_DTYPE = np.dtype(
    [("id", "<i4"), ("cls", "<u4"), ("position", "<u4"), ("start", "<u4"), ("end", "<u4"), ("byte_len", "<u4")]
)
TOKEN8_DTYPE = np.dtype([("id", "<i4"), ("packed", "<u4")])  # kgpu_token8: cls | chars << 2 | byte_len << 14
# kgpu_norm_edit and kgpu_span (include/kanpyo_gpu.h, "source alignment")
EDIT_DTYPE = np.dtype([("out_pos", "<u4"), ("src_pos", "<u4"), ("out_char", "<u4"), ("src_char", "<u4"),
                       ("out_len", "<u2"), ("src_len", "<u2"), ("out_chars", "<u2"), ("src_chars", "<u2")])
SPAN_DTYPE = np.dtype([("position", "<u4"), ("byte_len", "<u4"), ("start", "<u4"), ("end", "<u4")])
SENTENCE_DTYPE = np.dtype([("line", "<u8"), ("byte_start", "<u4"), ("char_start", "<u4")])   # kgpu_sentence (include/kanpyo_gpu.h, "sentences")


def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """np.empty in pinned host memory (kgpu_host_alloc); freed when the array (and its views) are collected."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if not np.isscalar(shape) else int(shape)
    nbytes = max(count * dt.itemsize, 1)
    L = _lib.lib()
    p = L.kgpu_host_alloc(nbytes)
    if not p:
        raise MemoryError(L.kgpu_last_error().decode("utf-8", "replace"))
    buf = (C.c_uint8 * nbytes).from_address(p)
    weakref.finalize(buf, L.kgpu_host_free, p)
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def pack_sentences(sentences: Sequence) -> tuple:
    """list of str/bytes -> (uint8 concatenation, uint64 offsets[n+1])."""
    enc = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in sentences]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        offs[1:] = np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.uint64, count=len(enc)))
    return np.frombuffer(b"".join(enc), dtype=np.uint8), offs


def packed_input(utf8, offsets) -> tuple:
    """(utf8, offsets) as the batch entries take them -> (uint8 array, uint64 array, n sentences, their bytes in all)."""
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    if n < 0:
        raise ValueError("offsets needs n+1 entries")
    return utf8, offsets, n, int(offsets[-1] - offsets[0]) if n else 0


def block_bytes(block) -> np.ndarray:
    """A block of input (bytes-like or uint8 array) as a contiguous uint8 array."""
    return np.frombuffer(bytes(block), dtype=np.uint8) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block, dtype=np.uint8)


def ptr(a: np.ndarray):
    """The address of an input array; NULL for an empty one."""
    return a.ctypes.data if a.size else None


def grown(rc: int, caps: tuple, reported: tuple, slack: int = 0):
    """THE retry rule.  -> the capacities of the one more call, or None: a call is repeated only when it answered KGPU_ERR_CAPACITY and reported
    a size beyond a capacity it was given; each capacity then becomes max(itself, reported + slack).  Any other failure raises here."""
    if rc == _lib.KGPU_ERR_CAPACITY and any(r > c for r, c in zip(reported, caps)):
        return tuple(max(c, r + slack) for r, c in zip(reported, caps))
    _lib.check(rc)
    return None


def device_call(attempt, caps: tuple, slack: int = 0, fixed: bool = False) -> tuple:
    """One stage of a device-resident call (normalise, tokenize, encode, pack): attempt(*caps) allocates what the capacities size, synchronizes,
    enqueues and syncs -> (rc, the sizes the sync reported, whatever it allocated).  -> (reported, allocated) of the attempt that fitted; `grown`
    alone decides whether there is one more.  fixed: the capacities are the caller's (a padded encode) -- KGPU_ERR_CAPACITY raises at once."""
    while True:
        rc, reported, made = attempt(*caps)
        more = _lib.check(rc) if fixed else grown(rc, caps, reported, slack)   # (check returns None)
        if more is None:
            return tuple(reported), made
        caps = more


def batch_call(entry, utf8, offsets, dtype, first_capacity, names, slack=0, alloc=np.empty, out=None, capacity=None):
    """One batch entry point: entry(utf8_ptr, offsets_ptr, n, units_ptr, capacity, unit_offsets_ptr, status_ptr, byref(got)) -> rc, the
    arguments in front of or between these bound by the caller.  -> (units[:got], unit_offsets[:n+1], status[:n]).
    dtype: the units'; first_capacity(total bytes, n) -> the units allocated for the first call; slack: added to a reported size; alloc: np.empty
    or pinned_empty; names: ("tokens[TOKEN_DTYPE]", "tok_offsets"), for the message about a bad out=.
    out=(units, unit_offsets, status): the caller's arrays, used as they are; they and an explicit `capacity` are never grown -- the library's
    KGPU_ERR_CAPACITY surfaces as KgpuError."""
    utf8, offsets, n, total = packed_input(utf8, offsets)
    if out is not None:
        units, uoff, status = out
        if units.dtype != dtype or uoff.dtype != np.uint64 or status.dtype != np.uint8 or uoff.size < n + 1 or status.size < n:
            raise ValueError(f"out=({names[0]}, {names[1]}[uint64 >= n+1], status[uint8 >= n])")
        cap = units.size
    else:
        cap = int(capacity) if capacity is not None else first_capacity(total, n)
        uoff = alloc(n + 1, dtype=np.uint64)
        status = alloc(max(n, 1), dtype=np.uint8)
    fixed = out is not None or capacity is not None
    got = C.c_uint64(0)
    while True:
        if out is None:
            units = alloc(max(cap, 1), dtype=dtype)
        status[: max(n, 1)] = 0
        rc = entry(ptr(utf8), offsets.ctypes.data, n, units.ctypes.data, cap, uoff.ctypes.data, status.ctypes.data, C.byref(got))
        more = _lib.check(rc) if fixed else grown(rc, (cap,), (got.value,), slack)   # (check returns None)
        if more is None:
            return units[: got.value], uoff[: n + 1], status[:n]
        (cap,) = more


def block_call(entry, block, dtype, first_capacities):
    """One raw-block entry point (the split and the trim run on the device): entry(src_ptr, len, units_ptr, capacity, unit_offsets_ptr,
    offsets_capacity, status_ptr, byref(n_lines), byref(got)) -> rc.  -> (units[:got], unit_offsets[:n_lines+1], status[:n_lines]).
    first_capacities(len) -> (capacity, offsets_capacity) of the first call; whichever was short grows to the size the library reports."""
    src = block_bytes(block)
    caps = first_capacities(src.size)
    n, got = C.c_uint64(0), C.c_uint64(0)
    while caps is not None:
        cap, ocap = caps
        units = np.empty(max(cap, 1), dtype=dtype)
        uoff = np.empty(ocap, dtype=np.uint64)
        status = np.zeros(ocap, dtype=np.uint8)
        rc = entry(ptr(src), src.size, units.ctypes.data, cap, uoff.ctypes.data, ocap, status.ctypes.data, C.byref(n), C.byref(got))
        caps = grown(rc, caps, (got.value, n.value + 1))
    return units[: got.value], uoff[: n.value + 1], status[: n.value]


def struct_dict(s: C.Structure) -> dict:
    """The fields of an info struct the library has filled in, without its `size` and `reserved`."""
    return {n: int(getattr(s, n)) for n, *_ in s._fields_ if n not in ("size", "reserved")}


class Handle:
    """An object of the library behind one opaque pointer.  A subclass names its destroy symbol and sets _h once its create call succeeded;
    close() is idempotent, and silent on an object whose constructor failed before that."""

    _destroy = None   # e.g. "kgpu_dict_destroy"
    _h = None

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            getattr(_lib.lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
