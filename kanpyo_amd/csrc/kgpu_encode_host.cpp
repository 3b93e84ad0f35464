// kanpyo_amd/csrc/kgpu_encode_host.cpp -- the vocabulary handle behind the vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids"; kgpu_encode.hip).
//
// Owns: kgpu_vocab_create / _destroy / _get_info (the two tables are built by build_vocab_table, kgpu_vocab_table.cpp, and uploaded once per handle); the
// encode's enqueue on a context (enqueue_encode: the renders' lines_report and lines_len, waited for by kgpu_ctx_sync_lines, which reports the ids),
// kgpu_encode_device; the host calls kgpu_encode_batch and kgpu_encode_text -- the lines calls' bodies (batch_lines, kgpu_host.cpp; text_lines,
// kgpu_split_host.cpp) with LinesChunk::vocab set, the chunk's output counted in 4-byte units; and the host-only test hook kgpu_debug_vocab_table.
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
    (void)hipFree(v->d_row_id); (void)hipFree(v->d_slots); (void)hipFree(v->d_arena);
    kgpu_words *w = v->words;
    delete v;
    words_release(w);
}

}  // namespace

extern "C" int kgpu_vocab_create(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_vocab_opts *opts,
                                 kgpu_vocab **out) {
    const char *who = "kgpu_vocab_create";
    if (!w || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    int rc;
    if ((rc = check_opts(opts, who))) return rc;
    kgpu_dict *d = w->dict;
    const size_t nk = (size_t)d->info.n_morphs;
    const bool need_keys = any_known_surface_row(w->h_rows, nk);
    if (need_keys) dict_key_table(d);
    VocabTables t;
    std::string err;
    if ((rc = build_vocab_table(w->h_rows.data(), w->h_rows.size(), nk, w->h_names.data(), need_keys ? d->key_bytes.data() : nullptr,
                                need_keys ? d->key_off.data() : nullptr, words, word_offsets, n_words, opts->unk_id, t, err))) {
        set_error("%s: %s", who, err.c_str());
        return rc;
    }
    HIPCHECK(hipSetDevice(d->device));
    kgpu_vocab *v = new kgpu_vocab();
    v->words = w;
    w->refs.fetch_add(1, std::memory_order_relaxed);
    v->flags = opts->flags; v->unk_id = opts->unk_id; v->bos_id = opts->bos_id; v->eos_id = opts->eos_id;
    v->n_words = n_words; v->table_slots = t.slots.size(); v->key_bytes = t.arena.size() - 16; v->rows_resolved = t.rows_resolved;
    const size_t row_bytes = std::max<size_t>(t.row_id.size() * 4, 16), slot_bytes = t.slots.size() * sizeof(VocabSlot);
    if (hipMalloc(&v->d_row_id, row_bytes) != hipSuccess || hipMalloc(&v->d_slots, slot_bytes) != hipSuccess || hipMalloc(&v->d_arena, t.arena.size()) != hipSuccess) {
        (void)hipGetLastError();
        free_vocab(v);
        set_error("%s: no device memory for %zu rows, %zu slots and %zu key bytes", who, t.row_id.size(), t.slots.size(), t.arena.size());
        return KGPU_ERR_HIP;
    }
    if ((!t.row_id.empty() && hipMemcpy(v->d_row_id, t.row_id.data(), t.row_id.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(v->d_slots, t.slots.data(), slot_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->d_arena, t.arena.data(), t.arena.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        free_vocab(v);
        set_error("%s: upload of the vocabulary tables failed", who);
        return KGPU_ERR_HIP;
    }
    *out = v;
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
                         uint64_t *d_id_offsets, const char *who) {
    if (v->words->dict != c->dict) { set_error("%s: the context's dictionary is not the vocabulary handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (width && (r.n > ~0ull / width || id_capacity < r.n * width)) {
        set_error("%s: id capacity %llu, the padded form needs n x width = %llu x %llu", who, (unsigned long long)id_capacity, (unsigned long long)r.n, (unsigned long long)width);
        return KGPU_ERR_INVALID_ARG;
    }
    EncodeArgs a{};
    if (int rc = records_batch(c, r, (size_t)r.n * 8 + 8, d_id_offsets, a.b)) return rc;
    a.w = word_table(v->words);
    a.row_id = (const int32_t *)v->d_row_id;
    a.slots = (const VocabSlot *)v->d_slots; a.slot_mask = (uint32_t)(v->table_slots - 1);
    a.arena = (const uint8_t *)v->d_arena;
    a.unk_id = v->unk_id; a.bos_id = v->bos_id; a.eos_id = v->eos_id; a.pad_id = pad_id;
    a.flags = v->flags;
    a.ids = d_ids; a.id_cap = id_capacity; a.width = width;
    return records_launched(c, launch_encode(a, c->stream), who, "encode", width ? ~0ull : id_capacity);   // (the padded form never reports KGPU_ERR_CAPACITY)
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

// ---- the host calls: the lines calls' bodies with the chunks' renderer set to the encode --------------------------------------------------------
extern "C" int kgpu_encode_batch(kgpu_vocab *v, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, int32_t *ids, uint64_t id_capacity,
                                 uint64_t *id_offsets, uint8_t *status, uint64_t *n_ids) {
    if (!v) { set_error("kgpu_encode_batch: null argument"); return KGPU_ERR_INVALID_ARG; }
    return batch_lines(v->words->dict, nullptr, v, "kgpu_encode_batch", utf8, offsets, n, (uint8_t *)ids, id_capacity, id_offsets, status, n_ids);
}

extern "C" int kgpu_encode_text(kgpu_vocab *v, const uint8_t *text, uint64_t len, int32_t *ids, uint64_t id_capacity, uint64_t *id_offsets,
                                uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_ids) {
    if (!v) { set_error("kgpu_encode_text: null argument"); return KGPU_ERR_INVALID_ARG; }
    return text_lines(v->words->dict, nullptr, v, "kgpu_encode_text", text, len, (uint8_t *)ids, id_capacity, id_offsets, offsets_capacity, status, n_lines, n_ids);
}

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
    const size_t rows_n = (size_t)(n_morphs + n_unk);
    std::vector<WordRow> rows(rows_n);
    uint64_t pool_len = 0;
    rc = kgpu_debug_word_table(known, known_len, unk, unk_len, n_morphs, n_unk, spec, (uint32_t *)rows.data(), nullptr, 0, &pool_len, nullptr);
    if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    std::vector<uint8_t> names((size_t)pool_len + 1);
    if ((rc = kgpu_debug_word_table(known, known_len, unk, unk_len, n_morphs, n_unk, spec, (uint32_t *)rows.data(), names.data(), pool_len, &pool_len, nullptr))) return rc;
    std::vector<uint8_t> keys(1);
    std::vector<uint64_t> key_off((size_t)n_morphs + 1, 0);
    const bool need_keys = any_known_surface_row(rows, (size_t)n_morphs);
    if (need_keys) {
        uint64_t klen = 0;
        rc = kgpu_debug_key_table(index_blob, blob_len, n_morphs, nullptr, 0, &klen, key_off.data());
        if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) { set_error("%s: the index blob does not parse", who); return rc; }
        keys.resize((size_t)klen + 1);
        if ((rc = kgpu_debug_key_table(index_blob, blob_len, n_morphs, keys.data(), klen, &klen, key_off.data()))) return rc;
    }
    VocabTables t;
    std::string err;
    if ((rc = build_vocab_table(rows.data(), rows.size(), (size_t)n_morphs, names.data(), need_keys ? keys.data() : nullptr, need_keys ? key_off.data() : nullptr,
                                words, word_offsets, n_words, opts->unk_id, t, err))) {
        set_error("%s: %s", who, err.c_str());
        return rc;
    }
    *n_slots = t.slots.size();
    *arena_len = t.arena.size() - 16;
    if (rows_resolved) *rows_resolved = t.rows_resolved;
    if (row_id && !t.row_id.empty()) std::memcpy(row_id, t.row_id.data(), t.row_id.size() * 4);
    if (t.slots.size() > slots_cap || *arena_len > arena_cap) { set_error("%s: buffers too small: %zu slots, %llu arena bytes", who, t.slots.size(), (unsigned long long)*arena_len); return KGPU_ERR_CAPACITY; }
    for (size_t i = 0; i < t.slots.size(); ++i) { slots[2 * i] = t.slots[i].tag; slots[2 * i + 1] = (uint64_t)(uint32_t)t.slots[i].id; }
    if (*arena_len) std::memcpy(arena, t.arena.data(), (size_t)*arena_len);
    return KGPU_OK;
}
