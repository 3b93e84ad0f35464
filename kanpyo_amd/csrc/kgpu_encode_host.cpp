// kanpyo_amd/csrc/kgpu_encode_host.cpp -- the vocabulary handle behind the vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids"; kgpu_encode.hip).
//
// Owns: kgpu_vocab_create / _destroy / _get_info (the two tables are built by build_vocab_table, kgpu_vocab_table.cpp, and uploaded once per handle);
// kgpu_vocab_create_wordpiece / kgpu_vocab_get_wordpiece_info (include/kanpyo_gpu.h, "WordPiece ids": the same handle with build_wordpiece_tables' tables,
// kgpu_wordpiece_table.cpp; enqueue_encode sends it to kgpu_wordpiece.hip's launcher, a plain handle to kgpu_encode.hip's as before); the
// encode's enqueue on a context (enqueue_encode: the renders' lines_report and lines_len, waited for by kgpu_ctx_sync_lines, which reports the ids),
// kgpu_encode_device and kgpu_encode_device_spans (include/kanpyo_gpu.h, "ids with spans": the same enqueue with the write kernels' SPANS instantiation); the host calls kgpu_encode_batch and kgpu_encode_text -- the lines calls' wrappers (batch_lines, kgpu_host.cpp; text_lines,
// kgpu_split_host.cpp) with the handle as the Renderer, the chunk's output counted in 4-byte units; and the host-only test hooks kgpu_debug_vocab_table,
// kgpu_debug_wordpiece_table, kgpu_debug_wordpiece_split and kgpu_debug_wordpiece_split_ends.
//
// AN ENCODE IS IDEMPOTENT, as a render is: queued behind a chunk's first pass it simply runs again when kgpu_ctx_sync had to rerun the chain
// (LinesChunk::finish) -- unlike a count, which cannot be taken back.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "kgpu_runtime.h"

extern "C" int kgpu_debug_key_table(const uint8_t *index_blob, size_t blob_len, uint64_t n_morphs, uint8_t *keys, uint64_t keys_cap, uint64_t *keys_len,
                                    uint64_t *key_offsets);
extern "C" int kgpu_debug_word_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                                     const kgpu_words_spec *spec, uint32_t *entries, uint8_t *pool, uint64_t pool_cap, uint64_t *pool_len, uint32_t *separator);

namespace {

int check_opts(const kgpu_vocab_opts *o, const char *who) {
    if (!o) { set_error("%s: null opts", who); return KGPU_ERR_INVALID_ARG; }
    if (o->size < sizeof(kgpu_vocab_opts)) { set_error("%s: opts.size %u, the struct has %zu bytes", who, o->size, sizeof(kgpu_vocab_opts)); return KGPU_ERR_INVALID_ARG; }
    if (o->flags & ~(KGPU_VOCAB_ADD_BOS | KGPU_VOCAB_ADD_EOS)) { set_error("%s: unknown flags %#x", who, o->flags); return KGPU_ERR_INVALID_ARG; }
    return KGPU_OK;
}

bool any_known_surface_row(const std::vector<WordRow> &rows, size_t nk) {
    for (size_t r = 0; r < nk && r < rows.size(); ++r)
        if (rows[r].len_flags & WORD_SURFACE) return true;
    return false;
}

void free_vocab(kgpu_vocab *v) {
    (void)hipSetDevice(v->words->dict->device);
    (void)hipFree(v->d_row_id); (void)hipFree(v->d_slots); (void)hipFree(v->d_arena); (void)hipFree(v->d_entry);
    (void)hipFree(v->d_cont_slots); (void)hipFree(v->d_cont_arena); (void)hipFree(v->d_wp_rows); (void)hipFree(v->d_piece_ids); (void)hipFree(v->d_piece_ends);
    kgpu_words *w = v->words;
    delete v;
    words_release(w);
}

}  // namespace

namespace {

// The WordPiece options as the tables take them: a null wp is "##", 100.
struct WpSpec { uint8_t prefix[8]; uint32_t prefix_len, max_chars; };
int check_wp(const kgpu_wordpiece_opts *wp, const char *who, WpSpec &o) {
    o = WpSpec{{'#', '#', 0, 0, 0, 0, 0, 0}, 2, WORDPIECE_DEFAULT_CHARS};
    if (!wp) return KGPU_OK;
    if (wp->size < sizeof(kgpu_wordpiece_opts)) { set_error("%s: wp.size %u, the struct has %zu bytes", who, wp->size, sizeof(kgpu_wordpiece_opts)); return KGPU_ERR_INVALID_ARG; }
    if (wp->prefix_len > WORDPIECE_MAX_PREFIX) { set_error("%s: prefix_len %u, at most %u", who, wp->prefix_len, WORDPIECE_MAX_PREFIX); return KGPU_ERR_INVALID_ARG; }
    if (wp->max_word_chars > WORDPIECE_MAX_CHARS) { set_error("%s: max_word_chars %u, at most %u", who, wp->max_word_chars, WORDPIECE_MAX_CHARS); return KGPU_ERR_INVALID_ARG; }
    std::memcpy(o.prefix, wp->prefix, 8);
    o.prefix_len = wp->prefix_len;
    o.max_chars = wp->max_word_chars ? wp->max_word_chars : WORDPIECE_DEFAULT_CHARS;
    return KGPU_OK;
}

// hipMalloc of at least 16 bytes and the upload of `bytes` of them
bool upload(void **d, const void *src, size_t bytes) {
    if (hipMalloc(d, std::max<size_t>(bytes, 16)) != hipSuccess) return false;
    return bytes == 0 || hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// kgpu_vocab_create (spec null) and kgpu_vocab_create_wordpiece: the tables on the host, the handle, one upload.
int create_vocab(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_vocab_opts *opts, const WpSpec *spec,
                 kgpu_vocab **out, const char *who) {
    kgpu_dict *d = w->dict;
    const size_t nk = (size_t)d->info.n_morphs;
    const bool need_keys = any_known_surface_row(w->h_rows, nk);
    if (need_keys) dict_key_table(d);
    const uint8_t *kb = need_keys ? d->key_bytes.data() : nullptr;
    const uint64_t *ko = need_keys ? d->key_off.data() : nullptr;
    WordpieceTables wt;
    VocabTables &t = wt.initial;
    std::string err;
    int rc = spec ? build_wordpiece_tables(w->h_rows.data(), w->h_rows.size(), nk, w->h_names.data(), kb, ko, words, word_offsets, n_words, opts->unk_id,
                                           spec->prefix, spec->prefix_len, spec->max_chars, wt, err)
                  : build_vocab_table(w->h_rows.data(), w->h_rows.size(), nk, w->h_names.data(), kb, ko, words, word_offsets, n_words, opts->unk_id, t, err);
    if (rc) { set_error("%s: %s", who, err.c_str()); return rc; }
    HIPCHECK(hipSetDevice(d->device));
    kgpu_vocab *v = new kgpu_vocab();
    v->words = w;
    w->refs.fetch_add(1, std::memory_order_relaxed);
    v->flags = opts->flags; v->unk_id = opts->unk_id; v->bos_id = opts->bos_id; v->eos_id = opts->eos_id;
    v->n_words = n_words; v->table_slots = t.slots.size(); v->key_bytes = t.arena.size() - 16; v->rows_resolved = t.rows_resolved;
    build_decode_entries(t, n_words, v->h_entry);   // (host memory, 4 bytes per word: kgpu_decode_device.cpp uploads it when a first decode asks for it)
    if (spec) { std::memcpy(v->prefix, spec->prefix, 8); v->prefix_len = spec->prefix_len; }
    bool ok = upload(&v->d_slots, t.slots.data(), t.slots.size() * sizeof(VocabSlot)) && upload(&v->d_arena, t.arena.data(), t.arena.size());
    if (!spec) ok = ok && upload(&v->d_row_id, t.row_id.data(), t.row_id.size() * 4);
    else {
        v->wordpiece = true; v->cont_shared = wt.shared;
        v->max_word_chars = spec->max_chars; v->initial_max = wt.initial_max; v->cont_max = wt.continuation_max();
        const VocabTables &ct = wt.continuation();
        v->wp.cont_words = wt.cont_words; v->wp.cont_table_slots = ct.slots.size(); v->wp.cont_key_bytes = ct.arena.size() - 16;
        v->wp.rows_whole = wt.rows_whole; v->wp.rows_split = wt.rows_split; v->wp.rows_unk = wt.rows_unk; v->wp.row_piece_ids = wt.piece_ids.size();
        v->wp.max_initial_bytes = wt.initial_max; v->wp.max_cont_bytes = wt.continuation_max();
        if (!wt.shared) ok = ok && upload(&v->d_cont_slots, ct.slots.data(), ct.slots.size() * sizeof(VocabSlot)) && upload(&v->d_cont_arena, ct.arena.data(), ct.arena.size());
        ok = ok && upload(&v->d_wp_rows, wt.rows.data(), wt.rows.size() * sizeof(WordpieceRow)) && upload(&v->d_piece_ids, wt.piece_ids.data(), wt.piece_ids.size() * 4) &&
                 upload(&v->d_piece_ends, wt.piece_ends.data(), wt.piece_ends.size() * sizeof(PieceEnd));   // (8 bytes per pooled id, for the span calls)
    }
    if (!ok) {
        (void)hipGetLastError();
        free_vocab(v);
        set_error("%s: no device memory for, or no upload of, the vocabulary tables: %zu rows, %zu slots and %zu key bytes", who, w->h_rows.size(), t.slots.size(), t.arena.size());
        return KGPU_ERR_HIP;
    }
    *out = v;
    return KGPU_OK;
}

}  // namespace

extern "C" int kgpu_vocab_create(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_vocab_opts *opts,
                                 kgpu_vocab **out) {
    const char *who = "kgpu_vocab_create";
    if (!w || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (int rc = check_opts(opts, who)) return rc;
    return create_vocab(w, words, word_offsets, n_words, opts, nullptr, out, who);
}

extern "C" int kgpu_vocab_create_wordpiece(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_vocab_opts *opts,
                                           const kgpu_wordpiece_opts *wp, kgpu_vocab **out) {
    const char *who = "kgpu_vocab_create_wordpiece";
    if (!w || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    WpSpec spec;
    int rc;
    if ((rc = check_opts(opts, who)) || (rc = check_wp(wp, who, spec))) return rc;
    return create_vocab(w, words, word_offsets, n_words, opts, &spec, out, who);
}

extern "C" int kgpu_vocab_get_wordpiece_info(const kgpu_vocab *v, kgpu_wordpiece_info *info) {
    const char *who = "kgpu_vocab_get_wordpiece_info";
    if (!v || !info || info->size < 8) { set_error("%s: null argument, or info.size not set", who); return KGPU_ERR_INVALID_ARG; }
    if (!v->wordpiece) { set_error("%s: a plain vocabulary", who); return KGPU_ERR_INVALID_ARG; }
    kgpu_wordpiece_info full = v->wp;
    full.size = (uint32_t)std::min<size_t>(info->size, sizeof full);
    full.reserved = 0;
    std::memcpy(info, &full, full.size);
    return KGPU_OK;
}

extern "C" void kgpu_vocab_destroy(kgpu_vocab *v) {
    if (v) free_vocab(v);
}

extern "C" int kgpu_vocab_get_info(const kgpu_vocab *v, kgpu_vocab_info *info) {
    if (!v || !info || info->size < 8) { set_error("kgpu_vocab_get_info: null argument, or info.size not set"); return KGPU_ERR_INVALID_ARG; }
    kgpu_vocab_info full{};
    full.size = (uint32_t)std::min<size_t>(info->size, sizeof full);
    full.n_words = v->n_words; full.table_slots = v->table_slots; full.key_bytes = v->key_bytes; full.rows_resolved = v->rows_resolved;
    std::memcpy(info, &full, full.size);
    return KGPU_OK;
}

// ---- the encode of a batch's records on a context --------------------------------------------------------------------------------------------
int kgpu::enqueue_encode(kgpu_ctx *c, const kgpu_vocab *v, const DeviceRecords &r, int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id,
                         uint64_t *d_id_offsets, const char *who, const SpanOut *spans) {
    if (v->words->dict != c->dict) { set_error("%s: the context's dictionary is not the vocabulary handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (width && (r.n > ~0ull / width || id_capacity < r.n * width)) {
        set_error("%s: id capacity %llu, the padded form needs n x width = %llu x %llu", who, (unsigned long long)id_capacity, (unsigned long long)r.n, (unsigned long long)width);
        return KGPU_ERR_INVALID_ARG;
    }
    if (v->wordpiece) {   // (the one place that tells the two kinds of handle apart: a plain handle runs exactly the kernels below)
        WordpieceSpanArgs a{};   // (without spans only its WordpieceArgs part is used)
        if (int rc = records_batch(c, r, (size_t)r.n * 8 + 8, d_id_offsets, a.b)) return rc;
        a.w = word_table(v->words);
        a.rows = (const WordpieceRow *)v->d_wp_rows; a.piece_ids = (const int32_t *)v->d_piece_ids;
        a.initial = ByteTable{(const VocabSlot *)v->d_slots, (uint32_t)(v->table_slots - 1), (const uint8_t *)v->d_arena, v->initial_max};
        a.cont = v->cont_shared ? a.initial : ByteTable{(const VocabSlot *)v->d_cont_slots, (uint32_t)(v->wp.cont_table_slots - 1), (const uint8_t *)v->d_cont_arena, v->cont_max};
        a.max_chars = v->max_word_chars;
        a.unk_id = v->unk_id; a.bos_id = v->bos_id; a.eos_id = v->eos_id; a.pad_id = pad_id;
        a.flags = v->flags;
        a.ids = d_ids; a.id_cap = id_capacity; a.width = width;
        if (!spans) return records_launched(c, launch_wordpiece(a, c->stream), who, "wordpiece", width ? ~0ull : id_capacity);
        a.o = *spans; a.piece_ends = (const PieceEnd *)v->d_piece_ends;
        return records_launched(c, launch_wordpiece_spans(a, c->stream), who, "wordpiece spans", width ? ~0ull : id_capacity);
    }
    EncodeSpanArgs a{};
    if (int rc = records_batch(c, r, (size_t)r.n * 8 + 8, d_id_offsets, a.b)) return rc;
    a.w = word_table(v->words);
    a.row_id = (const int32_t *)v->d_row_id;
    a.slots = (const VocabSlot *)v->d_slots; a.slot_mask = (uint32_t)(v->table_slots - 1);
    a.arena = (const uint8_t *)v->d_arena;
    a.unk_id = v->unk_id; a.bos_id = v->bos_id; a.eos_id = v->eos_id; a.pad_id = pad_id;
    a.flags = v->flags;
    a.ids = d_ids; a.id_cap = id_capacity; a.width = width;
    if (!spans) return records_launched(c, launch_encode(a, c->stream), who, "encode", width ? ~0ull : id_capacity);   // (the padded form never reports KGPU_ERR_CAPACITY)
    a.o = *spans;
    return records_launched(c, launch_encode_spans(a, c->stream), who, "encode spans", width ? ~0ull : id_capacity);
}

extern "C" int kgpu_encode_device(kgpu_ctx *c, const kgpu_vocab *v, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                  const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                                  int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id, uint64_t *d_id_offsets) {
    const char *who = "kgpu_encode_device";
    if (!c || !v || !d_offsets || !d_tok_offsets || !d_id_offsets || (n && (!d_utf8 || !d_tokens)) || (id_capacity && !d_ids)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if ((uintptr_t)d_ids & 3u) { set_error("%s: d_ids is not 4-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if (v->words->dict != c->dict) { set_error("%s: the context's dictionary is not the vocabulary handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_encode(c, v, DeviceRecords{d_utf8, d_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, d_ids, id_capacity, width, pad_id, d_id_offsets, who);
}

extern "C" int kgpu_encode_device_spans(kgpu_ctx *c, const kgpu_vocab *v, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                        const kgpu_token *d_tokens, const uint64_t *d_tok_offsets, const kgpu_norm_edit *d_edits, const uint64_t *d_edit_offsets,
                                        int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id, uint64_t *d_id_offsets,
                                        kgpu_span *d_spans, int32_t *d_token_index) {
    const char *who = "kgpu_encode_device_spans";
    if (!c || !v || !d_offsets || !d_tok_offsets || !d_id_offsets || !d_spans || (n && (!d_utf8 || !d_tokens)) || (id_capacity && !d_ids)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if ((d_edits == nullptr) != (d_edit_offsets == nullptr)) { set_error("%s: d_edits and d_edit_offsets are given together, or both NULL", who); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_ids & 3u) { set_error("%s: d_ids is not 4-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_spans & 15u) { set_error("%s: d_spans is not 16-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_token_index & 3u) { set_error("%s: d_token_index is not 4-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if (v->words->dict != c->dict) { set_error("%s: the context's dictionary is not the vocabulary handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    const SpanOut o{d_spans, d_token_index, d_edits, d_edit_offsets};
    return enqueue_encode(c, v, DeviceRecords{d_utf8, d_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, d_ids, id_capacity, width, pad_id, d_id_offsets, who, &o);
}

// ---- the host calls: the lines calls' bodies with the chunks' renderer set to the encode --------------------------------------------------------
extern "C" int kgpu_encode_batch(kgpu_vocab *v, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, int32_t *ids, uint64_t id_capacity,
                                 uint64_t *id_offsets, uint8_t *status, uint64_t *n_ids) {
    if (!v) { set_error("kgpu_encode_batch: null argument"); return KGPU_ERR_INVALID_ARG; }
    return batch_lines(v->words->dict, Renderer(v), "kgpu_encode_batch", utf8, offsets, n, (uint8_t *)ids, id_capacity, id_offsets, status, n_ids);
}

extern "C" int kgpu_encode_text(kgpu_vocab *v, const uint8_t *text, uint64_t len, int32_t *ids, uint64_t id_capacity, uint64_t *id_offsets,
                                uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_ids) {
    if (!v) { set_error("kgpu_encode_text: null argument"); return KGPU_ERR_INVALID_ARG; }
    return text_lines(v->words->dict, Renderer(v), "kgpu_encode_text", text, len, (uint8_t *)ids, id_capacity, id_offsets, offsets_capacity, status, n_lines, n_ids);
}

namespace {

// The hooks' host tables without a dictionary handle: the word table of the two feature blobs and the spec, and the id -> key table of the index blob.
struct HostRows { std::vector<WordRow> rows; std::vector<uint8_t> names, keys; std::vector<uint64_t> key_off; bool need_keys = false; };
int host_rows(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, const uint8_t *index_blob, size_t blob_len, uint64_t n_morphs, uint64_t n_unk,
              const kgpu_words_spec *spec, const char *who, HostRows &h) {
    int rc;
    h.rows.resize((size_t)(n_morphs + n_unk));
    uint64_t pool_len = 0;
    rc = kgpu_debug_word_table(known, known_len, unk, unk_len, n_morphs, n_unk, spec, (uint32_t *)h.rows.data(), nullptr, 0, &pool_len, nullptr);
    if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    h.names.resize((size_t)pool_len + 1);
    if ((rc = kgpu_debug_word_table(known, known_len, unk, unk_len, n_morphs, n_unk, spec, (uint32_t *)h.rows.data(), h.names.data(), pool_len, &pool_len, nullptr))) return rc;
    h.keys.assign(1, 0);
    h.key_off.assign((size_t)n_morphs + 1, 0);
    h.need_keys = any_known_surface_row(h.rows, (size_t)n_morphs);
    if (h.need_keys) {
        uint64_t klen = 0;
        rc = kgpu_debug_key_table(index_blob, blob_len, n_morphs, nullptr, 0, &klen, h.key_off.data());
        if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) { set_error("%s: the index blob does not parse", who); return rc; }
        h.keys.resize((size_t)klen + 1);
        if ((rc = kgpu_debug_key_table(index_blob, blob_len, n_morphs, h.keys.data(), klen, &klen, h.key_off.data()))) return rc;
    }
    return KGPU_OK;
}

// A byte table into the hooks' buffers: slots as 2 x slots_cap 64-bit words ({tag, id in the low half}), the arena without its spare bytes.
bool table_out(const VocabTables &t, uint64_t *slots, uint64_t slots_cap, uint64_t *n_slots, uint8_t *arena, uint64_t arena_cap, uint64_t *arena_len) {
    *n_slots = t.slots.size();
    *arena_len = t.arena.size() - 16;
    if (t.slots.size() > slots_cap || *arena_len > arena_cap) return false;
    for (size_t i = 0; i < t.slots.size(); ++i) { slots[2 * i] = t.slots[i].tag; slots[2 * i + 1] = (uint64_t)(uint32_t)t.slots[i].id; }
    if (*arena_len) std::memcpy(arena, t.arena.data(), (size_t)*arena_len);
    return true;
}

}  // namespace

// Test hook (host only, not in the header): the tables of kgpu_vocab_create without a device or a handle.  The two feature blobs and the spec as
// kgpu_debug_word_table takes them, the index blob as kgpu_debug_key_table takes it.  row_id: n_morphs + n_unk entries.  slots: 2 x slots_cap 64-bit words
// ({tag, id in the low half}); arena: arena_cap bytes.  *n_slots / *arena_len: the exact sizes; KGPU_ERR_CAPACITY when either buffer is too small (row_id
// and *rows_resolved are written all the same).
extern "C" int kgpu_debug_vocab_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, const uint8_t *index_blob, size_t blob_len,
                                      uint64_t n_morphs, uint64_t n_unk, const kgpu_words_spec *spec, const uint8_t *words, const uint64_t *word_offsets,
                                      uint64_t n_words, const kgpu_vocab_opts *opts, int32_t *row_id, uint64_t *slots, uint64_t slots_cap, uint64_t *n_slots,
                                      uint8_t *arena, uint64_t arena_cap, uint64_t *arena_len, uint64_t *rows_resolved) {
    const char *who = "kgpu_debug_vocab_table";
    int rc;
    if (!n_slots || !arena_len) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if ((rc = check_opts(opts, who))) return rc;
    HostRows h;
    if ((rc = host_rows(known, known_len, unk, unk_len, index_blob, blob_len, n_morphs, n_unk, spec, who, h))) return rc;
    VocabTables t;
    std::string err;
    if ((rc = build_vocab_table(h.rows.data(), h.rows.size(), (size_t)n_morphs, h.names.data(), h.need_keys ? h.keys.data() : nullptr, h.need_keys ? h.key_off.data() : nullptr,
                                words, word_offsets, n_words, opts->unk_id, t, err))) {
        set_error("%s: %s", who, err.c_str());
        return rc;
    }
    if (rows_resolved) *rows_resolved = t.rows_resolved;
    if (row_id && !t.row_id.empty()) std::memcpy(row_id, t.row_id.data(), t.row_id.size() * 4);
    if (!table_out(t, slots, slots_cap, n_slots, arena, arena_cap, arena_len)) { set_error("%s: buffers too small: %zu slots, %llu arena bytes", who, t.slots.size(), (unsigned long long)*arena_len); return KGPU_ERR_CAPACITY; }
    return KGPU_OK;
}

// Test hook (host only, not in the header): the tables of kgpu_vocab_create_wordpiece without a device or a handle; the dictionary side as
// kgpu_debug_vocab_table takes it.  sizes (in / out, 6 words): [0] initial slots, [1] initial arena bytes, [2] continuation slots, [3] continuation arena
// bytes, [4] row entries, [5] pool ids -- in: the capacities of the six buffers, out: the exact sizes; KGPU_ERR_CAPACITY (sizes and *info written) when one is
// too small.  rows: 2 x uint32 per entry ({first, count}).  With prefix_len == 0 the continuation buffers receive the shared table.  info: optional.
extern "C" int kgpu_debug_wordpiece_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, const uint8_t *index_blob, size_t blob_len,
                                          uint64_t n_morphs, uint64_t n_unk, const kgpu_words_spec *spec, const uint8_t *words, const uint64_t *word_offsets,
                                          uint64_t n_words, const kgpu_vocab_opts *opts, const kgpu_wordpiece_opts *wp, uint64_t *sizes, uint64_t *islots, uint8_t *iarena,
                                          uint64_t *cslots, uint8_t *carena, uint32_t *rows, int32_t *piece_ids, kgpu_wordpiece_info *info) {
    const char *who = "kgpu_debug_wordpiece_table";
    int rc;
    WpSpec ws;
    if (!sizes) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if ((rc = check_opts(opts, who)) || (rc = check_wp(wp, who, ws))) return rc;
    HostRows h;
    if ((rc = host_rows(known, known_len, unk, unk_len, index_blob, blob_len, n_morphs, n_unk, spec, who, h))) return rc;
    WordpieceTables t;
    std::string err;
    if ((rc = build_wordpiece_tables(h.rows.data(), h.rows.size(), (size_t)n_morphs, h.names.data(), h.need_keys ? h.keys.data() : nullptr, h.need_keys ? h.key_off.data() : nullptr,
                                     words, word_offsets, n_words, opts->unk_id, ws.prefix, ws.prefix_len, ws.max_chars, t, err))) {
        set_error("%s: %s", who, err.c_str());
        return rc;
    }
    const VocabTables &ct = t.continuation();
    if (info) {
        *info = kgpu_wordpiece_info{(uint32_t)sizeof(kgpu_wordpiece_info), 0, t.cont_words, ct.slots.size(), ct.arena.size() - 16, t.rows_whole, t.rows_split, t.rows_unk,
                                    t.piece_ids.size(), t.initial_max, t.continuation_max()};
    }
    const uint64_t cap[6] = {sizes[0], sizes[1], sizes[2], sizes[3], sizes[4], sizes[5]};
    bool ok = table_out(t.initial, islots, cap[0], &sizes[0], iarena, cap[1], &sizes[1]);
    ok = table_out(ct, cslots, cap[2], &sizes[2], carena, cap[3], &sizes[3]) && ok;
    sizes[4] = t.rows.size(); sizes[5] = t.piece_ids.size();
    if (!ok || sizes[4] > cap[4] || sizes[5] > cap[5]) { set_error("%s: buffers too small", who); return KGPU_ERR_CAPACITY; }
    if (!t.rows.empty()) std::memcpy(rows, t.rows.data(), t.rows.size() * sizeof(WordpieceRow));
    if (!t.piece_ids.empty()) std::memcpy(piece_ids, t.piece_ids.data(), t.piece_ids.size() * 4);
    return KGPU_OK;
}

// The body of the two split hooks below (ends null: the ids alone).
namespace {
int debug_split(const char *who, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_wordpiece_opts *wp, int32_t unk_id, const uint8_t *in,
                const uint64_t *in_offsets, uint64_t n, int32_t *ids, uint32_t *ends, uint64_t ids_cap, uint64_t *out_offsets, uint64_t *n_ids) {
    int rc;
    WpSpec ws;
    if (!n_ids || !out_offsets || (n && !in_offsets)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if ((rc = check_wp(wp, who, ws))) return rc;
    WordpieceTables t;
    std::string err;
    if ((rc = build_wordpiece_tables(nullptr, 0, 0, nullptr, nullptr, nullptr, words, word_offsets, n_words, unk_id, ws.prefix, ws.prefix_len, ws.max_chars, t, err))) {
        set_error("%s: %s", who, err.c_str());
        return rc;
    }
    std::vector<int32_t> all;
    std::vector<PieceEnd> all_ends;
    out_offsets[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (in_offsets[i + 1] < in_offsets[i] || in_offsets[i + 1] - in_offsets[i] >= (1ull << 32)) { set_error("%s: bad offsets at word %llu", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
        wordpiece_split(t, in + in_offsets[i], in_offsets[i + 1] - in_offsets[i], ws.max_chars, unk_id, all, ends ? &all_ends : nullptr);
        out_offsets[i + 1] = all.size();
    }
    *n_ids = all.size();
    if (all.size() > ids_cap) { set_error("%s: id buffer too small: need %zu, capacity %llu", who, all.size(), (unsigned long long)ids_cap); return KGPU_ERR_CAPACITY; }
    if (!all.empty()) std::memcpy(ids, all.data(), all.size() * 4);
    if (ends && !all_ends.empty()) std::memcpy(ends, all_ends.data(), all_ends.size() * sizeof(PieceEnd));
    return KGPU_OK;
}
}  // namespace

// Test hook (host only, not in the header; kanpyo_amd.Vocab.split_words): wordpiece_split over packed words (word i is in[in_offsets[i] .. in_offsets[i + 1])) with
// the tables of the list alone -> ragged ids: out_offsets has n + 1 entries, *n_ids is the exact count; KGPU_ERR_CAPACITY (nothing written to ids) when
// ids_cap is below it.
extern "C" int kgpu_debug_wordpiece_split(const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_wordpiece_opts *wp, int32_t unk_id,
                                          const uint8_t *in, const uint64_t *in_offsets, uint64_t n, int32_t *ids, uint64_t ids_cap, uint64_t *out_offsets,
                                          uint64_t *n_ids) {
    return debug_split("kgpu_debug_wordpiece_split", words, word_offsets, n_words, wp, unk_id, in, in_offsets, n, ids, nullptr, ids_cap, out_offsets, n_ids);
}

// Test hook (host only, not in the header; kanpyo_amd.vocab.split_words_ends): kgpu_debug_wordpiece_split that also gives, per id, where its piece ENDS inside
// its word -- ends: 2 x ids_cap uint32, {byte end, character end} per id, what the span calls' pool holds for a row-determined word (include/kanpyo_gpu.h,
// "ids with spans").  The one id of a word that gives unk_id ends where the word ends.  ends is required.
extern "C" int kgpu_debug_wordpiece_split_ends(const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_wordpiece_opts *wp, int32_t unk_id,
                                               const uint8_t *in, const uint64_t *in_offsets, uint64_t n, int32_t *ids, uint32_t *ends, uint64_t ids_cap,
                                               uint64_t *out_offsets, uint64_t *n_ids) {
    const char *who = "kgpu_debug_wordpiece_split_ends";
    if (!ends) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    return debug_split(who, words, word_offsets, n_words, wp, unk_id, in, in_offsets, n, ids, ends, ids_cap, out_offsets, n_ids);
}
