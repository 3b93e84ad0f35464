"""Model inputs (include/kanpyo_gpu.h, "model inputs"): ragged id sequences packed into padded rows [R, max_length] with token_type_ids and an
attention_mask -- sentence pairs, truncation, overlapping stride windows.  pack_host is the rule on the host (numpy in, numpy out, no device):
what DeviceContext.pack and Vocab.encode_pairs_tensor compute on the device is defined by it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._calls import SPAN_DTYPE

STRATEGIES = {"longest_first": _lib.KGPU_PACK_LONGEST_FIRST, "only_first": _lib.KGPU_PACK_ONLY_FIRST, "only_second": _lib.KGPU_PACK_ONLY_SECOND}


def pack_opts(max_length: int, stride: int = 0, truncation="only_second", windows: bool = True, cls_id: int = 0, sep_id: int = 0, pad_id: int = 0,
              trim_front: int = 0, trim_back: int = 0) -> "_lib.PackOpts":
    """kgpu_pack_opts.  truncation: "longest_first" / "only_first" / "only_second" or the header's 0 / 1 / 2 (ValueError for another name; the numbers
    and everything else are the library's to check)."""
    if isinstance(truncation, str):
        if truncation not in STRATEGIES:
            raise ValueError(f"unknown truncation {truncation!r}: longest_first, only_first or only_second")
        truncation = STRATEGIES[truncation]
    return _lib.PackOpts(C.sizeof(_lib.PackOpts), _lib.KGPU_PACK_WINDOWS if windows else 0, int(truncation), int(max_length), int(stride),
                         int(cls_id), int(sep_id), int(pad_id), int(trim_front), int(trim_back))


def pack_host(opts, ids_a, off_a, ids_b=None, off_b=None, spans_in=None, tix_in=None, row_capacity=None, type_ids=True, mask=True) -> dict:
    """kgpu_pack_host.  opts: pack_opts(...).  ids_a int32 with off_a uint64 [n + 1]; ids_b / off_b the same for pairs (None: singles; both id
    arrays are indexed by the same offsets and have the same size).  spans_in (SPAN_DTYPE or uint32 [.., 4]) and tix_in (int32): optional, carried
    along.  -> dict of input_ids, token_type_ids, attention_mask (int32 [R, max_length]; the two last only when asked for), spans, token_index (when
    given), row_offsets (uint64 [n + 1]) and status (uint8 [n]).  row_capacity None: as many rows as the rule makes; a number: that many, and
    KgpuError with KGPU_ERR_CAPACITY (err.rows: the count needed) when it is too small."""
    L = _lib.lib()
    ids_a = np.ascontiguousarray(ids_a, dtype=np.int32)
    off_a = np.ascontiguousarray(off_a, dtype=np.uint64)
    n = off_a.size - 1
    if n < 0:
        raise ValueError("off_a needs n + 1 entries")
    pair = off_b is not None
    if pair:
        ids_b = np.ascontiguousarray(ids_a if ids_b is None else ids_b, dtype=np.int32)
        off_b = np.ascontiguousarray(off_b, dtype=np.uint64)
        if off_b.size != n + 1 or ids_b.size != ids_a.size:
            raise ValueError("off_b has n + 1 entries, and ids_b the size of ids_a")
    if spans_in is not None:
        spans_in = np.ascontiguousarray(spans_in).view(np.uint32).reshape(-1, 4)
        if spans_in.shape[0] != ids_a.size:
            raise ValueError("spans_in has one span per id")
        spans_in = _aligned16(spans_in)
    if tix_in is not None:
        tix_in = np.ascontiguousarray(tix_in, dtype=np.int32)
        if tix_in.size != ids_a.size:
            raise ValueError("tix_in has one index per id")
    ML = int(opts.max_length)
    roff, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
    got = C.c_uint64(0)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731  (an empty array still has an address: NULL means "not given")
    cap = 0 if row_capacity is None else int(row_capacity)
    while True:
        rows = {"input_ids": np.empty((cap, ML), dtype=np.int32)}
        if type_ids:
            rows["token_type_ids"] = np.empty((cap, ML), dtype=np.int32)
        if mask:
            rows["attention_mask"] = np.empty((cap, ML), dtype=np.int32)
        if spans_in is not None:
            rows["spans"] = _aligned16(np.empty((cap * ML, 4), dtype=np.uint32), copy=False)
        if tix_in is not None:
            rows["token_index"] = np.empty((cap, ML), dtype=np.int32)
        rc = L.kgpu_pack_host(C.byref(opts), n, p(ids_a), p(off_a), p(ids_b) if pair else None, p(off_b) if pair else None, ids_a.size, p(spans_in), p(tix_in),
                              p(rows["input_ids"]), p(rows.get("token_type_ids")), p(rows.get("attention_mask")), p(rows.get("spans")), p(rows.get("token_index")),
                              cap, p(roff), p(status), C.byref(got))
        if rc == _lib.KGPU_ERR_CAPACITY and row_capacity is None and int(got.value) > cap:
            cap = int(got.value)
            continue
        if rc != _lib.KGPU_OK:
            err = _lib.KgpuError(rc, L.kgpu_last_error().decode("utf-8", "replace"))
            err.rows = int(got.value)
            raise err
        break
    R = int(got.value)
    out = {k: v[:R] for k, v in rows.items() if k != "spans"}
    if "spans" in rows:
        out["spans"] = rows["spans"][: R * ML].copy().view(SPAN_DTYPE).reshape(R, ML)
    out["row_offsets"], out["status"] = roff, status[:n]
    return out


def _aligned16(a: np.ndarray, copy: bool = True) -> np.ndarray:
    """The uint32 [k, 4] array at a 16-byte aligned address (kgpu_span arrays are 16-byte aligned; numpy promises no more than the item's alignment)."""
    if a.ctypes.data % 16 == 0:
        return a
    raw = np.empty(a.nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    out = raw[skip : skip + a.nbytes].view(np.uint32).reshape(a.shape)
    if copy:
        out[...] = a
    return out


def sample_of_row(row_offsets: np.ndarray) -> np.ndarray:
    """row_offsets [n + 1] -> the sample of every row (int64 [R]): the overflow_to_sample_mapping of other libraries."""
    ro = np.asarray(row_offsets, dtype=np.int64)
    return np.repeat(np.arange(ro.size - 1, dtype=np.int64), np.diff(ro))
