"""Measurement and test helpers over the library's kgpu_debug_* hooks (not part of the public header): native caller threads, and the host-side
merge of the multi-device call alone.  bench_extras.py, tools/ and the tests use them; the product modules do not."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib
from ._calls import TOKEN8_DTYPE, TOKEN_DTYPE


def concurrent_callers(tok, utf8: np.ndarray, offsets: np.ndarray, threads: int, calls_per_thread: int, n_pattern=(1,), expect=None) -> dict:
    """Measurement / test helper (kgpu_debug_concurrent_callers, not part of the public header): `threads` native host threads call
    kgpu_tokenize_batch in a loop -- thread t with n_pattern[t % len] sentences per call -- walking round the corpus.  expect=(tokens, offsets)
    of the whole corpus (e.g. the oracle's): every call's records are compared, `mismatching_calls` counts the ones that differ."""
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    L = _lib.lib()
    pat = np.ascontiguousarray(n_pattern, dtype=np.int32)
    stats = np.zeros(8, dtype=np.float64)
    et = eo = None
    if expect is not None:
        et = np.ascontiguousarray(expect[0]); eo = np.ascontiguousarray(expect[1], dtype=np.uint64)
        assert et.dtype == TOKEN_DTYPE
    _lib.check(L.kgpu_debug_concurrent_callers(tok.handle, utf8.ctypes.data, offsets.ctypes.data, offsets.size - 1, int(threads), int(calls_per_thread),
                                               pat.ctypes.data, pat.size, et.ctypes.data if et is not None else None, eo.ctypes.data if eo is not None else None, stats.ctypes.data))
    return {"wall_s": float(stats[0]), "p50_us": float(stats[1]), "p99_us": float(stats[2]), "mean_us": float(stats[3]), "mismatching_calls": int(stats[4]),
            "calls": int(stats[5]), "sentences": int(stats[6]), "sentences_per_s": float(stats[6] / stats[0]) if stats[0] > 0 else 0.0,
            "threads": int(threads), "n_pattern": [int(x) for x in pat], "caller_cpu_s": float(stats[7])}


def merge_shards(shards, cnt: int, slice_sentences: int = 2048, reps: int = 1, token_capacity: int | None = None, want_tokens: bool = True, compact: bool = False):
    """Measurement / test helper (kgpu_debug_merge_shards[_compact], not part of the public header; needs NO device): the host-side merge of
    kgpu_tokenize_batch_multi[_compact] over one super-chunk of `cnt` sentences.  shards[g] = (rec[TOKEN8_DTYPE], first[uint32 m x 2], toff[uint64 m + 1],
    status[uint8 m]) as shard g's compaction kernel leaves them; sentence j of the super-chunk is shard j mod G's local sentence j // G.
    -> (rc, tokens, tok_offsets, status, n_tokens, seconds for all `reps` repetitions); compact: tokens = (tokens8, first[cnt x 2])."""
    G = len(shards)
    L = _lib.lib()
    vp = C.c_void_p
    keep = [[np.ascontiguousarray(a, dtype=dt) for a, dt in zip(sh, (TOKEN8_DTYPE, np.uint32, np.uint64, np.uint8))] for sh in shards]
    arr = lambda k: (vp * G)(*[sh[k].ctypes.data for sh in keep])
    total = sum(int(sh[2][-1]) for sh in keep)
    cap = total if token_capacity is None else int(token_capacity)
    tokens = np.zeros(max(cap, 1), dtype=TOKEN8_DTYPE if compact else TOKEN_DTYPE)
    toff = np.zeros(cnt + 1, dtype=np.uint64)
    status = np.full(max(cnt, 1), 255, dtype=np.uint8)
    n_tok, secs = C.c_uint64(0), C.c_double(0)
    head = (G, cnt, arr(0), arr(1), arr(2), arr(3), int(slice_sentences), int(reps), tokens.ctypes.data if want_tokens else None)
    tail = (cap, toff.ctypes.data, status.ctypes.data, C.byref(n_tok), C.byref(secs))
    if compact:
        first = np.full((max(cnt, 1), 2), 0xABABABAB, dtype=np.uint32)
        rc = L.kgpu_debug_merge_shards_compact(*head, first.ctypes.data, *tail)
        return rc, (tokens[: min(cap, total)], first[:cnt]), toff, status[:cnt], int(n_tok.value), float(secs.value)
    rc = L.kgpu_debug_merge_shards(*head, *tail)
    return rc, tokens[: min(cap, total)], toff, status[:cnt], int(n_tok.value), float(secs.value)


def merge_bench(G: int = 8, sentences_per_shard: int = 8192, tokens_per_sentence: int = 32, reps: int = 20, compact: bool = False) -> dict:
    """The rate of that merge alone on this host's CPUs (bench.py's `multi_merge` entry): G synthetic shard blocks of a super-chunk, every sentence
    `tokens_per_sentence` records.  Per sentence the merge reads 8 t + 17 bytes and writes 24 t + 9 (t tokens): the 24-byte expansion is a
    memory-bandwidth job, so the rate is quoted beside a plain copy of the same number of bytes by the same worker threads' count of NumPy threads."""
    cnt = G * sentences_per_shard
    rng = np.random.default_rng(5)
    shards = []
    for g in range(G):
        m = sentences_per_shard
        toff = (np.arange(m + 1, dtype=np.uint64) * np.uint64(tokens_per_sentence))
        nt = int(toff[-1])
        rec = np.zeros(nt, dtype=TOKEN8_DTYPE)
        rec["id"] = rng.integers(1, 390000, size=nt)
        rec["packed"] = 1 | (2 << 2) | (6 << 14)
        shards.append((rec, np.zeros((m, 2), dtype=np.uint32), toff, np.zeros(m, dtype=np.uint8)))
    merge_shards(shards, cnt, reps=2, compact=compact)
    rc, _, _, _, n_tok, secs = merge_shards(shards, cnt, reps=reps, compact=compact)
    _lib.check(rc)
    moved = reps * ((n_tok * 16 + cnt * 34) if compact else (n_tok * 32 + cnt * 26))
    a = np.ones(n_tok * 24 // 8, dtype=np.uint64); b = np.empty_like(a)
    b[:] = a
    t0 = time.perf_counter()
    for _ in range(5):
        b[:] = a
    copy_gbs = 5 * a.nbytes * 2 / (time.perf_counter() - t0) / 1e9
    return {"sentences_per_s": reps * cnt / secs, "G": G, "sentences_per_super_chunk": cnt, "tokens_per_sentence": n_tok / cnt,
            "bytes_moved_GB_per_s": moved / secs / 1e9, "one_thread_copy_GB_per_s": copy_gbs, "record_bytes": 8 if compact else 24,
            "what": "kgpu_tokenize_batch_multi" + ("_compact" if compact else "") + "'s merge alone (no device): G shards' 8-byte records -> the caller's order as " + ("8" if compact else "24") + "-byte records + global offsets + "
                    "status bytes; slice totals from the shards' offset tables on the calling thread, one worker-pool task per 2048 sentences walks the G "
                    "cursors (no division per sentence); the calling thread's own share is O(slices x G)"}
