"""ctypes binding of libkanpyo_gpu.so (include/kanpyo_gpu.h).  Fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KGPU_LIB: another build of the same library (kernel experiments, tools/ only); the default is the in-tree build
LIB_PATH = os.environ.get("KGPU_LIB") or os.path.join(_HERE, "libkanpyo_gpu.so")

KGPU_OK = 0
KGPU_ERR_INVALID_ARG = 1
KGPU_ERR_BAD_DICT = 2
KGPU_ERR_HIP = 3
KGPU_ERR_CAPACITY = 4
KGPU_ERR_NO_DEVICE = 5
KGPU_ERR_INTERNAL = 6
KGPU_SENT_OK = 0
KGPU_SENT_INVALID_UTF8 = 1
KGPU_SENT_NO_SCRATCH = 2
KGPU_SENT_TRUNCATED = 3
KGPU_SENT_NOT_NORMALIZED = 4   # the normalise calls: a segment was oversize, the line is unchanged
NORMALIZE_NFC, NORMALIZE_NFKC = 1, 2
KGPU_NORMALIZE_MAX_SEGMENT = 64

# every symbol include/kanpyo_gpu.h declares
SYMBOLS = [
    "kgpu_last_error", "kgpu_device_count", "kgpu_dict_create", "kgpu_dict_destroy", "kgpu_dict_get_info",
    "kgpu_tokenize_batch", "kgpu_ctx_create", "kgpu_ctx_destroy", "kgpu_tokenize_device", "kgpu_tokenize_device_compact", "kgpu_expand_tokens", "kgpu_ctx_sync",
    "kgpu_ctx_set_profiling", "kgpu_ctx_set_ablation", "kgpu_ctx_get_profile", "kgpu_ctx_get_routing", "kgpu_ctx_get_plan", "kgpu_ctx_get_work", "kgpu_ctx_get_phase_cycles", "kgpu_index_build", "kgpu_free",
    "kgpu_host_alloc", "kgpu_host_free", "kgpu_lattice_dump", "kgpu_lattice_free",
    "kgpu_dict_get_routing", "kgpu_tokenize_batch_multi", "kgpu_tokenize_batch_multi_compact", "kgpu_multi_create", "kgpu_multi_destroy", "kgpu_multi_tokenize_device", "kgpu_multi_sync",
    "kgpu_dict_set_features", "kgpu_tokenize_batch_lines", "kgpu_format_lines_device", "kgpu_ctx_sync_lines", "kgpu_split_lines",
    "kgpu_split_lines_device", "kgpu_ctx_sync_split", "kgpu_tokenize_text_lines", "kgpu_graphviz_batch",
    "kgpu_words_create", "kgpu_words_destroy", "kgpu_tokenize_batch_words", "kgpu_tokenize_text_words", "kgpu_format_words_device",
    "kgpu_counts_create", "kgpu_counts_destroy", "kgpu_counts_reset", "kgpu_counts_get_info", "kgpu_count_batch", "kgpu_count_text",
    "kgpu_count_words_device", "kgpu_ctx_sync_count", "kgpu_counts_read",
    "kgpu_vocab_create", "kgpu_vocab_destroy", "kgpu_vocab_get_info", "kgpu_encode_batch", "kgpu_encode_text", "kgpu_encode_device",
    "kgpu_vocab_create_wordpiece", "kgpu_vocab_get_wordpiece_info",
    "kgpu_normalize_unicode_version", "kgpu_normalize_host", "kgpu_normalize_batch", "kgpu_normalize_text", "kgpu_normalize_device", "kgpu_ctx_sync_normalize",
    "kgpu_normalize_host_aligned", "kgpu_normalize_batch_aligned", "kgpu_normalize_text_aligned", "kgpu_normalize_device_aligned", "kgpu_ctx_sync_normalize_aligned",
    "kgpu_source_spans_host", "kgpu_source_spans_device", "kgpu_source_spans_batch",
    "kgpu_encode_device_spans",
    "kgpu_pack_host", "kgpu_pack_device",
    "kgpu_decode_host", "kgpu_decode_device", "kgpu_decode_batch",
    "kgpu_nbest_host", "kgpu_tokenize_batch_nbest",
    "kgpu_marginals_host", "kgpu_samples_host", "kgpu_prob_exp_host", "kgpu_prob_log_host", "kgpu_tokenize_batch_marginals", "kgpu_tokenize_batch_samples",
    "kgpu_mode_host", "kgpu_tokenize_batch_mode",
    "kgpu_split_sentences_host", "kgpu_split_sentences_batch", "kgpu_split_sentences_device", "kgpu_ctx_sync_sentences",
    "kgpu_userdict_create", "kgpu_userdict_destroy", "kgpu_userdict_get_info", "kgpu_userdict_host", "kgpu_tokenize_batch_user",
]
KGPU_VOCAB_ADD_BOS, KGPU_VOCAB_ADD_EOS = 1, 2
KGPU_COUNTS_DEFAULT_SLOTS, KGPU_COUNTS_DEFAULT_KEY_BYTES = 1 << 22, 256 << 20
KGPU_WORDS_SURFACE = -1
KGPU_WORDS_ALL, KGPU_WORDS_DROP, KGPU_WORDS_KEEP = 0, 1, 2
KGPU_PACK_WINDOWS = 1
KGPU_PACK_LONGEST_FIRST, KGPU_PACK_ONLY_FIRST, KGPU_PACK_ONLY_SECOND = 0, 1, 2
KGPU_PACK_OK, KGPU_PACK_CUT, KGPU_PACK_NO_ROOM = 0, 1, 2
KGPU_DECODE_OK, KGPU_DECODE_BAD_ID, KGPU_DECODE_MAX_SKIP = 0, 1, 8
KGPU_NBEST_MAX = 64
KGPU_MARGINAL_BEST, KGPU_MARGINAL_ALL, KGPU_SAMPLES_MAX, KGPU_THETA_DEFAULT = 0, 1, 256, 0.75 / 800.0
KGPU_THETA_MAX = 2.0**64
KGPU_MODE_NORMAL, KGPU_MODE_SEARCH, KGPU_MODE_EXTENDED = 0, 1, 2
KGPU_SENTENCES_NO_BRACKETS, KGPU_SENTENCES_MAX_TERMINATORS = 1, 16
KGPU_CLASS_USER, KGPU_USERDICT_MAX_KEY_CHARS, KGPU_USERDICT_MAX_KEY_BYTES = 3, 64, 255


def normalize_form(form) -> int:
    """"NFC" / "NFKC" (any case), or the header's 1 / 2 -> KGPU_NORMALIZE_*; ValueError otherwise."""
    key = form.upper() if isinstance(form, str) else form
    if key in ("NFC", NORMALIZE_NFC):
        return NORMALIZE_NFC
    if key in ("NFKC", NORMALIZE_NFKC):
        return NORMALIZE_NFKC
    raise ValueError(f"unknown normalisation form {form!r}: NFC or NFKC")


def kernel_source_hash() -> str:
    """sha256[:16] over every source and header the library is built from (csrc/*.hip, *.cpp, *.h, *.inc, sorted, and the public header).
    Profile-derived files under profiles/ record it, bench.py compares: a counter file measured on other code says so (`stale`)."""
    import glob
    import hashlib

    csrc = os.path.join(_HERE, "csrc")
    names = sorted(os.path.basename(p) for ext in ("hip", "cpp", "h", "inc") for p in glob.glob(os.path.join(csrc, "*." + ext)))
    h = hashlib.sha256()
    for name in names + ["../../include/kanpyo_gpu.h"]:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


class KgpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kgpu error {code}: {msg}")
        self.code = code


class DictBlobs(C.Structure):
    _fields_ = [
        (n, t)
        for name in ("index", "connection", "morph", "unk", "char_category", "invoke", "group")
        for n, t in ((name + "_p", C.c_void_p), (name + "_len", C.c_size_t))
    ]


class DictInfo(C.Structure):
    _fields_ = [
        ("da_len", C.c_uint64), ("n_morphs", C.c_uint64), ("n_unk_morphs", C.c_uint64), ("conn_rows", C.c_uint64),
        ("conn_cols", C.c_uint64), ("device_bytes", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class Profile(C.Structure):  # kgpu_profile: 24 bytes, frozen
    _fields_ = [("launches", C.c_uint64), ("tokenize_ms", C.c_double), ("aux_ms", C.c_double)]


class Routing(C.Structure):  # kgpu_routing: read with its size, fields are only ever appended
    _fields_ = [("batches", C.c_uint64), ("sentences", C.c_uint64), ("deferred", C.c_uint64 * 4), ("redone", C.c_uint64 * 4),
                ("long_launches", C.c_uint64), ("arena_regrows", C.c_uint64), ("first_ms", C.c_double),
                ("small_calls", C.c_uint64), ("small_fallbacks", C.c_uint64), ("window_reruns", C.c_uint64), ("tail_reruns", C.c_uint64),
                ("combined_calls", C.c_uint64), ("combined_launches", C.c_uint64), ("window_handed", C.c_uint64 * 10)]


class PlanInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("compute_units", "pool_lds_bytes", "pool_wavefronts", "pool_workgroups_per_cu", "pool_max_pages",
                                          "long_lds_bytes", "long_workgroups_per_cu", "long_workgroups", "window_lds_bytes", "window_workgroups_per_cu", "window_workgroups",
                                          "streams", "long_streams", "window_first_bytes")] + [("reserved", C.c_uint32 * 2)]


class LatticeNode(C.Structure):
    _fields_ = [("id", C.c_int32), ("cls", C.c_uint32), ("byte_pos", C.c_uint32), ("char_pos", C.c_uint32), ("end_char", C.c_uint32),
                ("byte_len", C.c_uint32), ("left_id", C.c_int16), ("right_id", C.c_int16), ("cost", C.c_int16), ("reserved", C.c_int16),
                ("dp", C.c_int32), ("pre", C.c_int32)]


class LatticeOut(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_positions", C.c_uint64), ("nodes", C.POINTER(LatticeNode)),
                ("edge_offsets", C.POINTER(C.c_uint32)), ("edge_nodes", C.POINTER(C.c_uint32))]


class Token(C.Structure):  # kgpu_token
    _fields_ = [("id", C.c_int32), ("cls", C.c_uint32), ("position", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("byte_len", C.c_uint32)]


class Token8(C.Structure):  # kgpu_token8
    _fields_ = [("id", C.c_int32), ("packed", C.c_uint32)]


class NormEdit(C.Structure):  # kgpu_norm_edit: 24 bytes, one per segment of a line that normalisation changed
    _fields_ = [("out_pos", C.c_uint32), ("src_pos", C.c_uint32), ("out_char", C.c_uint32), ("src_char", C.c_uint32),
                ("out_len", C.c_uint16), ("src_len", C.c_uint16), ("out_chars", C.c_uint16), ("src_chars", C.c_uint16)]


class Span(C.Structure):  # kgpu_span: kgpu_token's position, byte_len, start and end in source coordinates
    _fields_ = [("position", C.c_uint32), ("byte_len", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32)]


class WordsSpec(C.Structure):  # kgpu_words_spec
    _fields_ = [("size", C.c_uint32), ("field", C.c_int32), ("filter", C.c_uint32), ("separator", C.c_uint32),
                ("names", C.c_void_p), ("name_offsets", C.c_void_p), ("n_names", C.c_uint64)]


class CountsOpts(C.Structure):  # kgpu_counts_opts
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("table_slots", C.c_uint64), ("key_bytes", C.c_uint64)]


class CountsInfo(C.Structure):  # kgpu_counts_info: read with its size, fields are only ever appended
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("tokens_counted", C.c_uint64), ("overflow_tokens", C.c_uint64), ("sentences", C.c_uint64),
                ("table_slots", C.c_uint64), ("table_slots_used", C.c_uint64), ("key_bytes", C.c_uint64), ("key_bytes_used", C.c_uint64)]


class VocabOpts(C.Structure):  # kgpu_vocab_opts
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("unk_id", C.c_int32), ("bos_id", C.c_int32), ("eos_id", C.c_int32)]


class VocabInfo(C.Structure):  # kgpu_vocab_info: read with its size, fields are only ever appended
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("n_words", C.c_uint64), ("table_slots", C.c_uint64), ("key_bytes", C.c_uint64),
                ("rows_resolved", C.c_uint64)]


class WordpieceOpts(C.Structure):  # kgpu_wordpiece_opts
    _fields_ = [("size", C.c_uint32), ("max_word_chars", C.c_uint32), ("prefix_len", C.c_uint32), ("prefix", C.c_uint8 * 8)]


class WordpieceInfo(C.Structure):  # kgpu_wordpiece_info: read with its size, fields are only ever appended
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32)] + [(n, C.c_uint64) for n in (
        "cont_words", "cont_table_slots", "cont_key_bytes", "rows_whole", "rows_split", "rows_unk", "row_piece_ids", "max_initial_bytes", "max_cont_bytes")]


class PackOpts(C.Structure):  # kgpu_pack_opts
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("strategy", C.c_uint32), ("max_length", C.c_uint32), ("stride", C.c_uint32),
                ("cls_id", C.c_int32), ("sep_id", C.c_int32), ("pad_id", C.c_int32), ("trim_front", C.c_uint32), ("trim_back", C.c_uint32)]


class DecodeOpts(C.Structure):  # kgpu_decode_opts
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("sep_len", C.c_uint32), ("sep", C.c_uint8 * 8), ("n_skip", C.c_uint32),
                ("skip_ids", C.c_int32 * KGPU_DECODE_MAX_SKIP)]


class ModeOpts(C.Structure):  # kgpu_mode_opts
    _fields_ = [("mode", C.c_uint32), ("kanji_length", C.c_uint32), ("kanji_penalty", C.c_uint32), ("other_length", C.c_uint32),
                ("other_penalty", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class UserdictInfo(C.Structure):  # kgpu_userdict_info
    _fields_ = [("entries", C.c_uint64), ("keys", C.c_uint64), ("longest_key", C.c_uint64), ("device_bytes", C.c_uint64)]


class SentenceOpts(C.Structure):  # kgpu_sentence_opts
    _fields_ = [("flags", C.c_uint32), ("n_terminators", C.c_uint32), ("terminators", C.c_uint32 * 16), ("reserved", C.c_uint32 * 2)]


class Sentence(C.Structure):  # kgpu_sentence: 16 bytes, one per sentence
    _fields_ = [("line", C.c_uint64), ("byte_start", C.c_uint32), ("char_start", C.c_uint32)]


def sentence_opts(terminators=None, brackets=True) -> SentenceOpts:
    """terminators: None (the default set), a str or an iterable of scalar values; brackets=False: no enclosing depth.  What does not fit the struct is a
    ValueError; what the rule forbids (White_Space, a bracket, ...) is the library's KGPU_ERR_INVALID_ARG."""
    cps = [] if terminators is None else [ord(c) if isinstance(c, str) else int(c) for c in terminators]
    if terminators is not None and not cps:
        raise ValueError("terminators: an empty set (None selects the default set)")
    if len(cps) > KGPU_SENTENCES_MAX_TERMINATORS:
        raise ValueError(f"terminators: {len(cps)} given, at most {KGPU_SENTENCES_MAX_TERMINATORS}")
    o = SentenceOpts()
    o.flags = 0 if brackets else KGPU_SENTENCES_NO_BRACKETS
    o.n_terminators = len(cps)
    for k, cp in enumerate(cps):
        if not 0 <= cp <= 0xFFFFFFFF:
            raise ValueError(f"terminators: {cp!r} is no scalar value")
        o.terminators[k] = cp
    return o


class Work(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("sentences", "B", "C", "T", "N", "E", "K")]


_lib = None


def lib():
    """Load the in-tree HIP extension; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C kanpyo_amd/csrc). "
                "kanpyo_amd has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.kgpu_last_error.restype = C.c_char_p
        L.kgpu_device_count.restype = C.c_int
        L.kgpu_dict_create.argtypes = [C.POINTER(DictBlobs), C.c_int, C.POINTER(vp)]
        L.kgpu_dict_destroy.argtypes = [vp]
        L.kgpu_dict_destroy.restype = None
        L.kgpu_dict_get_info.argtypes = [vp, C.POINTER(DictInfo)]
        L.kgpu_tokenize_batch.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_ctx_create.argtypes = [vp, vp, C.POINTER(vp)]
        L.kgpu_ctx_destroy.argtypes = [vp]
        L.kgpu_ctx_destroy.restype = None
        L.kgpu_tokenize_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp]
        L.kgpu_tokenize_device_compact.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
        L.kgpu_expand_tokens.argtypes = [vp, vp, vp, C.c_uint64, vp]
        L.kgpu_expand_tokens.restype = None
        L.kgpu_ctx_sync.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.kgpu_ctx_set_profiling.argtypes = [vp, C.c_int]
        L.kgpu_ctx_set_ablation.argtypes = [vp, C.c_int]
        L.kgpu_ctx_get_profile.argtypes = [vp, C.POINTER(Profile), C.c_int]
        L.kgpu_ctx_get_routing.argtypes = [vp, C.POINTER(Routing), C.c_size_t, C.c_int]
        L.kgpu_dict_get_routing.argtypes = [vp, C.POINTER(Routing), C.c_size_t, C.c_int]
        L.kgpu_ctx_get_plan.argtypes = [vp, C.POINTER(PlanInfo), C.c_size_t]
        L.kgpu_ctx_get_work.argtypes = [vp, C.POINTER(Work), C.c_int]
        L.kgpu_ctx_get_phase_cycles.argtypes = [vp, C.POINTER(C.c_uint64 * 10), C.c_int]
        L.kgpu_index_build.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.kgpu_free.argtypes = [vp]
        L.kgpu_free.restype = None
        L.kgpu_host_alloc.argtypes = [C.c_uint64]
        L.kgpu_host_alloc.restype = vp
        L.kgpu_host_free.argtypes = [vp]
        L.kgpu_host_free.restype = None
        L.kgpu_lattice_dump.argtypes = [vp, vp, C.c_uint64, C.POINTER(LatticeOut)]
        L.kgpu_lattice_free.argtypes = [C.POINTER(LatticeOut)]
        L.kgpu_lattice_free.restype = None
        L.kgpu_tokenize_batch_multi.argtypes = [C.POINTER(vp), C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_tokenize_batch_multi_compact.argtypes = [C.POINTER(vp), C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_multi_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp)]
        L.kgpu_multi_destroy.argtypes = [vp]
        L.kgpu_multi_destroy.restype = None
        L.kgpu_multi_tokenize_device.argtypes = [vp, C.c_int] + [vp] * 9
        L.kgpu_multi_sync.argtypes = [vp, C.c_int, vp]
        L.kgpu_dict_set_features.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        L.kgpu_tokenize_batch_lines.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_format_lines_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp]
        L.kgpu_ctx_sync_lines.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.kgpu_split_lines.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.kgpu_split_lines_device.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64]
        L.kgpu_ctx_sync_split.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_tokenize_text_lines.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_graphviz_batch.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_words_create.argtypes = [vp, C.POINTER(WordsSpec), C.POINTER(vp)]
        L.kgpu_words_destroy.argtypes = [vp]
        L.kgpu_words_destroy.restype = None
        L.kgpu_tokenize_batch_words.argtypes = L.kgpu_tokenize_batch_lines.argtypes
        L.kgpu_tokenize_text_words.argtypes = L.kgpu_tokenize_text_lines.argtypes
        L.kgpu_format_words_device.argtypes = [vp] + L.kgpu_format_lines_device.argtypes
        L.kgpu_counts_create.argtypes = [vp, C.POINTER(CountsOpts), C.POINTER(vp)]
        L.kgpu_counts_destroy.argtypes = [vp]
        L.kgpu_counts_destroy.restype = None
        L.kgpu_counts_reset.argtypes = [vp]
        L.kgpu_counts_get_info.argtypes = [vp, C.POINTER(CountsInfo)]
        L.kgpu_count_batch.argtypes = [vp, vp, vp, C.c_uint64, vp]
        L.kgpu_count_text.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.kgpu_count_words_device.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp]
        L.kgpu_ctx_sync_count.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.kgpu_counts_read.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_vocab_create.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(VocabOpts), C.POINTER(vp)]
        L.kgpu_vocab_destroy.argtypes = [vp]
        L.kgpu_vocab_destroy.restype = None
        L.kgpu_vocab_get_info.argtypes = [vp, C.POINTER(VocabInfo)]
        L.kgpu_encode_batch.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_encode_text.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_encode_device.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int32, vp]
        L.kgpu_debug_vocab_table.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(WordsSpec), vp, vp, C.c_uint64,
                                             C.POINTER(VocabOpts), vp, vp, C.c_uint64, C.POINTER(C.c_uint64), vp, C.c_uint64, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64)]
        L.kgpu_vocab_create_wordpiece.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(VocabOpts), C.POINTER(WordpieceOpts), C.POINTER(vp)]
        L.kgpu_vocab_get_wordpiece_info.argtypes = [vp, C.POINTER(WordpieceInfo)]
        L.kgpu_normalize_unicode_version.argtypes = []
        L.kgpu_normalize_unicode_version.restype = C.c_char_p
        L.kgpu_normalize_host.argtypes = [C.c_int, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
        L.kgpu_normalize_batch.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        L.kgpu_normalize_text.argtypes = [vp, C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_normalize_device.argtypes = [vp, C.c_int, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
        L.kgpu_ctx_sync_normalize.argtypes = [vp, C.POINTER(C.c_uint64)]
        edits_out = [vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]   # edits, edit_capacity, edit_offsets, n_edits
        L.kgpu_normalize_host_aligned.argtypes = L.kgpu_normalize_host.argtypes + [vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.kgpu_normalize_batch_aligned.argtypes = L.kgpu_normalize_batch.argtypes + edits_out
        L.kgpu_normalize_text_aligned.argtypes = L.kgpu_normalize_text.argtypes + edits_out
        L.kgpu_normalize_device_aligned.argtypes = L.kgpu_normalize_device.argtypes + [vp, C.c_uint64, vp]
        L.kgpu_ctx_sync_normalize_aligned.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_source_spans_host.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
        L.kgpu_source_spans_host.restype = None
        L.kgpu_source_spans_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64]
        L.kgpu_source_spans_batch.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp]
        L.kgpu_debug_wordpiece_table.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(WordsSpec), vp, vp, C.c_uint64,
                                                 C.POINTER(VocabOpts), C.POINTER(WordpieceOpts), vp, vp, vp, vp, vp, vp, vp, C.POINTER(WordpieceInfo)]
        L.kgpu_encode_device_spans.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int32, vp, vp, vp]
        pack = [C.POINTER(PackOpts), C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp]
        L.kgpu_pack_host.argtypes = pack + [C.POINTER(C.c_uint64)]
        L.kgpu_pack_device.argtypes = [vp] + pack
        decode = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(DecodeOpts), vp, C.c_uint64, vp, vp]   # ids, id_offsets, n, width, opts, text, capacity, text_offsets, status
        L.kgpu_decode_host.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32] + decode + [C.POINTER(C.c_uint64)]
        L.kgpu_decode_device.argtypes = [vp, vp] + decode
        L.kgpu_decode_batch.argtypes = [vp] + decode + [C.POINTER(C.c_uint64)]
        nbest_out = [vp, C.c_uint64, vp, vp, C.c_uint64]   # tokens, token_capacity, tok_offsets, costs, path_capacity
        L.kgpu_nbest_host.argtypes = [C.POINTER(LatticeOut), vp, C.c_uint64, C.c_uint64, C.c_uint32] + nbest_out + [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kgpu_tokenize_batch_nbest.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        u64p, lat_in = C.POINTER(C.c_uint64), [C.POINTER(LatticeOut), vp, C.c_uint64, C.c_uint64, C.c_double]   # lattice, conn, rows, cols, theta
        L.kgpu_marginals_host.argtypes = lat_in + [C.c_uint32, C.c_double, vp, C.c_uint64, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), u64p]
        L.kgpu_samples_host.argtypes = lat_in + [C.c_uint32, C.c_uint64, C.c_uint64] + nbest_out + [u64p, u64p]
        L.kgpu_prob_exp_host.argtypes = L.kgpu_prob_log_host.argtypes = [vp, C.c_uint64, vp]
        L.kgpu_prob_exp_host.restype = L.kgpu_prob_log_host.restype = None
        L.kgpu_debug_prob_device.argtypes = [C.c_int, C.c_uint32, vp, C.c_uint64, vp]
        L.kgpu_tokenize_batch_marginals.argtypes = [vp, vp, vp, C.c_uint64, C.c_double, C.c_uint32, C.c_double, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, u64p]
        L.kgpu_tokenize_batch_samples.argtypes = [vp, vp, vp, C.c_uint64, C.c_double, C.c_uint32, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, u64p, u64p]
        L.kgpu_mode_host.argtypes = [C.POINTER(LatticeOut), vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.POINTER(ModeOpts), vp, C.c_uint64, u64p, C.POINTER(C.c_int32)]
        L.kgpu_tokenize_batch_mode.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(ModeOpts), vp, C.c_uint64, vp, vp, vp, u64p]
        sent_out = [C.POINTER(SentenceOpts), vp, vp, vp, C.c_uint64]   # opts, out, out_offsets, sents, sent_capacity
        L.kgpu_split_sentences_host.argtypes = [vp, vp, C.c_uint64] + sent_out + [u64p]
        L.kgpu_split_sentences_batch.argtypes = [vp, vp, vp, C.c_uint64] + sent_out + [u64p]
        L.kgpu_split_sentences_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64] + sent_out
        L.kgpu_ctx_sync_sentences.argtypes = [vp, u64p, u64p]
        entries = [vp, vp, vp, vp, vp, C.c_uint64]   # keys, key_offsets, left_id, right_id, cost, E
        L.kgpu_userdict_create.argtypes = [vp] + entries + [C.POINTER(vp)]
        L.kgpu_userdict_destroy.argtypes = [vp]
        L.kgpu_userdict_destroy.restype = None
        L.kgpu_userdict_get_info.argtypes = [vp, C.POINTER(UserdictInfo)]
        L.kgpu_userdict_host.argtypes = [C.POINTER(LatticeOut), vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp] + entries + [C.POINTER(ModeOpts), vp, C.c_uint64, u64p, C.POINTER(C.c_int32)]
        L.kgpu_tokenize_batch_user.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(ModeOpts), vp, C.c_uint64, vp, vp, vp, u64p]
        L.kgpu_debug_userdict_hash.argtypes = [vp, C.c_uint32]
        L.kgpu_debug_userdict_hash.restype = C.c_uint32
        L.kgpu_debug_userdict_slots.argtypes = [C.c_uint64]
        L.kgpu_debug_userdict_slots.restype = C.c_uint64
        L.kgpu_debug_wordpiece_split_ends.argtypes = [vp, vp, C.c_uint64, C.POINTER(WordpieceOpts), C.c_int32, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        L.kgpu_debug_wordpiece_split.argtypes = [vp, vp, C.c_uint64, C.POINTER(WordpieceOpts), C.c_int32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        L.kgpu_debug_counts_order.argtypes = [vp, vp, vp, C.c_uint64] + L.kgpu_counts_read.argtypes[1:]
        L.kgpu_debug_key_table.argtypes = [vp, C.c_size_t, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
        L.kgpu_debug_word_table.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(WordsSpec), vp, vp, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.kgpu_debug_feature_pool.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        L.kgpu_debug_label_pool.argtypes = L.kgpu_debug_feature_pool.argtypes
        L.kgpu_debug_concurrent_callers.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
        shards = [C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_uint64, C.c_int]
        L.kgpu_debug_merge_shards.argtypes = shards + [vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.kgpu_debug_merge_shards_compact.argtypes = shards + [vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def check(rc: int):
    if rc != KGPU_OK:
        raise KgpuError(rc, lib().kgpu_last_error().decode("utf-8", "replace"))
