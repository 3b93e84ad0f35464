"""Device-resident entry points (include/kanpyo_gpu.h: kgpu_ctx_*, kgpu_tokenize_device).

Inputs already in HBM, outputs left in HBM: what bench.py times and what the
multi-GPU gather (kanpyo_amd/dist.py) consumes.  Pointers cross as plain
integers (e.g. torch.Tensor.data_ptr()); torch itself is not imported here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._calls import TOKEN_DTYPE, Handle, struct_dict

PROFILE_OFF, PROFILE_EVENTS, PROFILE_WORK, PROFILE_SAMPLED, PROFILE_NO_T = 0, 1, 2, 4, 8
STAGE_ALL, STAGE_LATTICE, STAGE_GATHER, STAGE_VITERBI = 0, 5, 6, 7  # kgpu_ctx_set_ablation


class DeviceContext(Handle):
    """One HIP stream + scratch arena; not thread-safe, make one per thread / per queue slot."""

    _destroy = "kgpu_ctx_destroy"

    def __init__(self, tokenizer, stream_ptr: int | None = None):
        self._tok = tokenizer  # keeps the dictionary alive
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_ctx_create(tokenizer.handle, C.c_void_p(stream_ptr) if stream_ptr else None, C.byref(h)))
        self._h = h

    def tokenize(self, d_utf8: int, d_offsets: int, n: int, total_bytes: int, d_tokens: int, token_capacity: int,
                 d_tok_offsets: int, d_status: int):
        """Enqueue one batch (asynchronous)."""
        _lib.check(_lib.lib().kgpu_tokenize_device(
            self._h, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, total_bytes, C.c_void_p(d_tokens), token_capacity,
            C.c_void_p(d_tok_offsets), C.c_void_p(d_status)))

    def tokenize_compact(self, d_utf8: int, d_offsets: int, n: int, total_bytes: int, d_tokens8: int, token_capacity: int,
                         d_first: int, d_tok_offsets: int, d_status: int):
        """Same batch, results as 8-byte kgpu_token8 records + the first token's (position, start) per sentence: a third of
        the volume for whatever moves them next (PCIe, the xGMI gather); expand_tokens() restores the 24-byte records."""
        _lib.check(_lib.lib().kgpu_tokenize_device_compact(
            self._h, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, total_bytes, C.c_void_p(d_tokens8), token_capacity,
            C.c_void_p(d_first), C.c_void_p(d_tok_offsets), C.c_void_p(d_status)))

    def _sync(self, entry: str, results: int = 1, raises: bool = True) -> tuple:
        """The sync family's one body: wait through `entry` -> (fits, its `results` 64-bit results...).  KGPU_ERR_CAPACITY raises like every
        other failure, or with raises=False gives fits False and the sizes the entry reported."""
        out = [C.c_uint64(0) for _ in range(results)]
        rc = getattr(_lib.lib(), entry)(self._h, *map(C.byref, out))
        if raises or rc != _lib.KGPU_ERR_CAPACITY:
            _lib.check(rc)
        return (rc == _lib.KGPU_OK,) + tuple(int(v.value) for v in out)

    def sync(self) -> int:
        """Wait for the enqueued batch; returns its dense token count."""
        return self._sync("kgpu_ctx_sync")[1]

    def try_sync(self) -> tuple:
        """-> (fits, tokens): sync without the exception for a token capacity that was too small."""
        return self._sync("kgpu_ctx_sync", raises=False)

    def format_lines(self, d_utf8: int, d_offsets: int, n: int, d_tokens: int, d_tok_offsets: int, d_text: int, text_capacity: int, d_text_offsets: int):
        """kgpu_format_lines_device: enqueue the `kanpyo tokenize` lines of records a synced batch left in HBM (the handle needs set_features)."""
        _lib.check(_lib.lib().kgpu_format_lines_device(
            self._h, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets), C.c_void_p(d_text),
            text_capacity, C.c_void_p(d_text_offsets)))

    def format_words(self, words, d_utf8: int, d_offsets: int, n: int, d_tokens: int, d_tok_offsets: int, d_text: int, text_capacity: int, d_text_offsets: int):
        """kgpu_format_words_device: enqueue the wakati lines (one line per sentence: its kept words, separated) of records a synced batch left in
        HBM, by a Words handle of this context's tokenizer (Tokenizer.words); sync_lines waits for it."""
        _lib.check(_lib.lib().kgpu_format_words_device(
            self._h, words.handle, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets), C.c_void_p(d_text),
            text_capacity, C.c_void_p(d_text_offsets)))

    def sync_lines(self) -> int:
        """Wait for the enqueued render (lines or words) or encode; returns its byte count, or the encode's id count."""
        return self._sync("kgpu_ctx_sync_lines")[1]

    def count_words(self, counts, d_utf8: int, d_offsets: int, n: int, d_tokens: int, d_tok_offsets: int):
        """kgpu_count_words_device: enqueue the word counts of records a synced batch left in HBM into a WordCounts handle of this context's
        tokenizer (Words.counter); sync_count waits for it."""
        _lib.check(_lib.lib().kgpu_count_words_device(
            self._h, counts.handle, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets)))

    def sync_count(self) -> int:
        """Wait for the enqueued count; returns the tokens it added.  KgpuError with KGPU_ERR_CAPACITY: some found no room (overflow_tokens)."""
        return self._sync("kgpu_ctx_sync_count")[1]

    def encode(self, vocab, d_utf8: int, d_offsets: int, n: int, d_tokens: int, d_tok_offsets: int, d_ids: int, id_capacity: int, d_id_offsets: int,
               width: int = 0, pad_id: int = 0):
        """kgpu_encode_device: enqueue the vocabulary ids (int32) of records a synced batch left in HBM, by a Vocab of this context's tokenizer.
        width 0: ragged, d_ids holds the sequences back to back; width w: padded, d_ids is n x w (id_capacity >= n * w), rows cut after w
        elements and filled with pad_id.  d_id_offsets: n + 1 uint64, the exclusive scan of the untruncated lengths.  sync_lines waits for it
        and returns d_id_offsets[n]."""
        _lib.check(_lib.lib().kgpu_encode_device(
            self._h, vocab.handle, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets), C.c_void_p(d_ids),
            id_capacity, width, pad_id, C.c_void_p(d_id_offsets)))

    def encode_spans(self, vocab, d_utf8: int, d_offsets: int, n: int, d_tokens: int, d_tok_offsets: int, d_ids: int, id_capacity: int, d_id_offsets: int,
                     d_spans: int, d_token_index: int = 0, d_edits: int = 0, d_edit_offsets: int = 0, width: int = 0, pad_id: int = 0):
        """kgpu_encode_device_spans: encode() that also leaves, for element e of d_ids, its source span (16-byte kgpu_span; d_spans 16-byte aligned,
        id_capacity entries) in d_spans[e] and the index of its token among the sentence's records in d_token_index[e] (int32, id_capacity entries; 0:
        not wanted); bos, eos and pad get zeros and -1.  d_edits / d_edit_offsets (both or neither): the edit records an aligned normalisation of the
        same lines left in HBM -- the spans are then in SOURCE coordinates.  sync_lines waits for it and returns d_id_offsets[n]."""
        _lib.check(_lib.lib().kgpu_encode_device_spans(
            self._h, vocab.handle, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets),
            C.c_void_p(d_edits) if d_edits else None, C.c_void_p(d_edit_offsets) if d_edit_offsets else None, C.c_void_p(d_ids), id_capacity, width, pad_id,
            C.c_void_p(d_id_offsets), C.c_void_p(d_spans), C.c_void_p(d_token_index) if d_token_index else None))

    def pack(self, opts, n: int, d_ids_a: int, d_off_a: int, n_ids_in: int, d_input_ids: int, row_capacity: int, d_row_offsets: int, d_status: int,
             d_ids_b: int = 0, d_off_b: int = 0, d_type_ids: int = 0, d_mask: int = 0, d_spans_in: int = 0, d_tix_in: int = 0, d_spans: int = 0, d_tix: int = 0):
        """kgpu_pack_device: enqueue the model inputs (include/kanpyo_gpu.h, "model inputs") of ragged ids an encode left in HBM -- rows [R, max_length]
        of input_ids and, where a pointer is given, token_type_ids, attention_mask (int32), spans (16-byte kgpu_span, 16-byte aligned) and token
        indices (int32), row_capacity rows each; d_row_offsets: n + 1 uint64, d_status: n bytes.  opts: pack.pack_opts(...).  d_ids_b / d_off_b:
        the second sequences of pairs (0: singles; d_off_b may be d_off_a + 8 n when 2 n sequences were encoded as one batch).  d_spans_in /
        d_tix_in: what encode_spans left beside the ids.  sync_lines (try_sync_lines) waits for it and returns the rows, written or needed."""
        p = lambda v: C.c_void_p(v) if v else None   # noqa: E731
        _lib.check(_lib.lib().kgpu_pack_device(
            self._h, C.byref(opts), n, p(d_ids_a), p(d_off_a), p(d_ids_b), p(d_off_b), n_ids_in, p(d_spans_in), p(d_tix_in), p(d_input_ids), p(d_type_ids),
            p(d_mask), p(d_spans), p(d_tix), row_capacity, p(d_row_offsets), p(d_status)))

    def decode(self, vocab, d_ids: int, d_id_offsets: int, n: int, d_text: int, text_capacity: int, d_text_offsets: int, d_status: int, width: int = 0, opts=None):
        """kgpu_decode_device: enqueue the text (include/kanpyo_gpu.h, "text from ids") of n sequences of int32 ids in HBM, by a Vocab of this context's
        tokenizer -- one line per sequence, packed in d_text, its uint64 offsets (n + 1) in d_text_offsets and a status byte per sequence in d_status.
        d_id_offsets (n + 1 uint64) with width 0: ragged; d_id_offsets 0 with width w: n rows of w ids.  opts: decode.decode_opts(...) (None: one space,
        no skip list).  sync_lines (try_sync_lines) waits for it and returns the bytes, written or needed."""
        p = lambda v: C.c_void_p(v) if v else None   # noqa: E731
        _lib.check(_lib.lib().kgpu_decode_device(
            self._h, vocab.handle, p(d_ids), p(d_id_offsets), n, width, C.byref(opts) if opts is not None else None, p(d_text), text_capacity,
            p(d_text_offsets), p(d_status)))

    def try_sync_lines(self) -> tuple:
        """-> (fits, units): sync_lines without the exception for a capacity that was too small (nothing was written then)."""
        return self._sync("kgpu_ctx_sync_lines", raises=False)

    def normalize(self, d_utf8: int, d_offsets: int, n: int, d_text: int, text_capacity: int, d_text_offsets: int, d_status: int, form="NFKC"):
        """kgpu_normalize_device: enqueue NFC / NFKC of n lines in HBM -> the normalised lines packed in d_text (up to 11 times the input's bytes;
        no overlap with d_utf8), their uint64 offsets in d_text_offsets (n + 1) and a status byte per line in d_status: the buffers tokenize takes
        next.  sync_normalize waits for it."""
        _lib.check(_lib.lib().kgpu_normalize_device(
            self._h, _lib.normalize_form(form), C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_text), text_capacity,
            C.c_void_p(d_text_offsets), C.c_void_p(d_status)))

    def sync_normalize(self) -> int:
        """Wait for the enqueued normalisation; returns its byte count.  KgpuError with KGPU_ERR_CAPACITY: text_capacity was too small (nothing
        was written); try_sync_normalize returns the size instead."""
        return self._sync("kgpu_ctx_sync_normalize")[1]

    def try_sync_normalize(self) -> tuple:
        """-> (fits, bytes): sync_normalize without the exception for a capacity that was too small."""
        return self._sync("kgpu_ctx_sync_normalize", raises=False)

    def normalize_aligned(self, d_utf8: int, d_offsets: int, n: int, d_text: int, text_capacity: int, d_text_offsets: int, d_status: int,
                          d_edits: int, edit_capacity: int, d_edit_offsets: int, form="NFKC"):
        """kgpu_normalize_device_aligned: normalize() that also leaves the lines' edit records (24-byte kgpu_norm_edit, at most one per input byte)
        in d_edits and their uint64 offsets (n + 1) in d_edit_offsets.  sync_normalize_aligned waits for it."""
        _lib.check(_lib.lib().kgpu_normalize_device_aligned(
            self._h, _lib.normalize_form(form), C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, C.c_void_p(d_text), text_capacity,
            C.c_void_p(d_text_offsets), C.c_void_p(d_status), C.c_void_p(d_edits), edit_capacity, C.c_void_p(d_edit_offsets)))

    def sync_normalize_aligned(self) -> tuple:
        """Wait for the enqueued aligned normalisation -> (bytes, edits).  KgpuError with KGPU_ERR_CAPACITY: either capacity was too small
        (nothing was written); try_sync_normalize_aligned returns the sizes instead."""
        return self._sync("kgpu_ctx_sync_normalize_aligned", 2)[1:]

    def try_sync_normalize_aligned(self) -> tuple:
        """-> (fits, bytes, edits): sync_normalize_aligned without the exception for a capacity that was too small."""
        return self._sync("kgpu_ctx_sync_normalize_aligned", 2, raises=False)

    def source_spans(self, d_tokens: int, d_tok_offsets: int, n: int, d_edits: int, d_edit_offsets: int, d_spans: int, span_capacity: int):
        """kgpu_source_spans_device: enqueue the source spans (16-byte kgpu_span, d_spans[k] for d_tokens[k]; d_spans 16-byte aligned) of records a
        synced batch left in HBM, through the edit records an aligned normalisation left there.  sync_lines waits for it."""
        _lib.check(_lib.lib().kgpu_source_spans_device(
            self._h, C.c_void_p(d_tokens), C.c_void_p(d_tok_offsets), n, C.c_void_p(d_edits), C.c_void_p(d_edit_offsets), C.c_void_p(d_spans), span_capacity))

    def split_lines(self, d_in: int, len: int, d_out: int, d_offsets: int, offsets_capacity: int):
        """kgpu_split_lines_device: enqueue read_line + trim_end over a block in HBM -> the trimmed lines packed in d_out (len bytes suffice,
        no overlap with d_in) and their uint64 offsets in d_offsets."""
        _lib.check(_lib.lib().kgpu_split_lines_device(
            self._h, C.c_void_p(d_in), len, C.c_void_p(d_out), C.c_void_p(d_offsets), offsets_capacity))

    def sync_split(self) -> tuple:
        """Wait for the enqueued split; returns (n_lines, n_bytes): d_offsets holds n_lines + 1 entries, d_out n_bytes bytes."""
        return self._sync("kgpu_ctx_sync_split", 2)[1:]

    def split_sentences(self, d_utf8: int, d_offsets: int, n: int, total_bytes: int, d_out: int, d_out_offsets: int, d_sents: int, sent_capacity: int, opts=None):
        """kgpu_split_sentences_device: enqueue the sentence split (include/kanpyo_gpu.h, "sentences") of n lines in HBM -> the sentences packed in
        d_out (total_bytes suffice, no overlap with the text), their uint64 offsets in d_out_offsets (sent_capacity + 1) and a 16-byte kgpu_sentence
        each in d_sents (16-byte aligned): the buffers tokenize takes next.  opts: _lib.sentence_opts(...) (None: the defaults).  sync_sentences
        waits for it."""
        _lib.check(_lib.lib().kgpu_split_sentences_device(
            self._h, C.c_void_p(d_utf8), C.c_void_p(d_offsets), n, total_bytes, C.byref(opts) if opts is not None else None, C.c_void_p(d_out),
            C.c_void_p(d_out_offsets), C.c_void_p(d_sents) if d_sents else None, sent_capacity))

    def sync_sentences(self) -> tuple:
        """Wait for the enqueued sentence split -> (sentences, bytes).  KgpuError with KGPU_ERR_CAPACITY: sent_capacity was too small (nothing was
        written); try_sync_sentences returns the count instead."""
        return self._sync("kgpu_ctx_sync_sentences", 2)[1:]

    def try_sync_sentences(self) -> tuple:
        """-> (fits, sentences, bytes): sync_sentences without the exception for a capacity that was too small."""
        return self._sync("kgpu_ctx_sync_sentences", 2, raises=False)

    def set_profiling(self, mode: int):
        _lib.check(_lib.lib().kgpu_ctx_set_profiling(self._h, int(mode)))

    def profile(self, reset: bool = True) -> dict:
        """Event timings (kgpu_profile) and routing counters (kgpu_routing) in one dict."""
        p, r = _lib.Profile(), _lib.Routing()
        _lib.check(_lib.lib().kgpu_ctx_get_profile(self._h, C.byref(p), int(reset)))
        _lib.check(_lib.lib().kgpu_ctx_get_routing(self._h, C.byref(r), C.sizeof(r), int(reset)))
        return {"launches": int(p.launches), "tokenize_ms": float(p.tokenize_ms), "aux_ms": float(p.aux_ms),
                "batches": int(r.batches), "sentences": int(r.sentences), "deferred": [int(x) for x in r.deferred],
                "redone": [int(x) for x in r.redone], "long_launches": int(r.long_launches),
                "arena_regrows": int(r.arena_regrows), "first_ms": float(r.first_ms),
                "small_calls": int(r.small_calls), "small_fallbacks": int(r.small_fallbacks), "window_reruns": int(r.window_reruns), "tail_reruns": int(r.tail_reruns),
                "window_handed": [int(x) for x in r.window_handed]}

    def plan(self) -> dict:
        """The launch plan (kgpu_plan_info): LDS bytes per workgroup and resident workgroups per CU of both kernels."""
        p = _lib.PlanInfo()
        _lib.check(_lib.lib().kgpu_ctx_get_plan(self._h, C.byref(p), C.sizeof(p)))
        return struct_dict(p)

    def set_ablation(self, stop_after_stage: int):
        """Measurement only: following batches stop after the given stage (STAGE_*), zero tokens; 0 = off."""
        _lib.check(_lib.lib().kgpu_ctx_set_ablation(self._h, int(stop_after_stage)))

    def work(self, reset: bool = True) -> dict:
        w = _lib.Work()
        _lib.check(_lib.lib().kgpu_ctx_get_work(self._h, C.byref(w), int(reset)))
        return struct_dict(w)

    def phase_cycles(self, reset: bool = True) -> dict:
        """Per-phase shader-clock cycles of the LDS kernel, summed over sentences (PROFILE_WORK runs)."""
        arr = (C.c_uint64 * 10)()
        _lib.check(_lib.lib().kgpu_ctx_get_phase_cycles(self._h, C.byref(arr), int(reset)))
        names = ["load", "decode", "walk", "scan", "emit", "gather", "sweep", "backtrace_tokens", "sentences", "spare"]
        return {n: int(arr[i]) for i, n in enumerate(names)}


def expand_tokens(tokens8, tok_offsets, first):
    """kgpu_expand_tokens: 8-byte records (uint32 [T, 2] or uint64 [T]) + token offsets [n + 1] + first [n, 2] -> TOKEN_DTYPE [T]
    (host side, numpy arrays)."""
    t8 = np.ascontiguousarray(tokens8).view(np.uint32).reshape(-1, 2)
    toff = np.ascontiguousarray(tok_offsets, dtype=np.uint64)
    fs = np.ascontiguousarray(first, dtype=np.uint32).reshape(-1)
    n = toff.size - 1
    out = np.empty(int(toff[n] - toff[0]), dtype=TOKEN_DTYPE)
    if out.size:
        _lib.lib().kgpu_expand_tokens(t8[int(toff[0]):].ctypes.data, toff.ctypes.data, fs.ctypes.data, n, out.ctypes.data)
    return out
