// kanpyo_amd/csrc/kgpu_words_host.cpp -- the words handle behind the wakati output (include/kanpyo_gpu.h, "wakati-gaki"; kgpu_words.hip).
//
// Owns: the check of a kgpu_words_spec, kgpu_words_create / kgpu_words_destroy (the per-row entries and the name pool are built by
// build_word_table, kgpu_features.cpp, and uploaded once per handle), the render's enqueue on a context (enqueue_words),
// kgpu_format_words_device, and the host-only test hook kgpu_debug_word_table.  The host calls kgpu_tokenize_batch_words and
// kgpu_tokenize_text_words are their _lines counterparts with the handle as the Renderer (kgpu_host.cpp, kgpu_split_host.cpp).
#include <algorithm>
#include <cstring>
#include <vector>

#include "kgpu_runtime.h"

// The spec as kgpu_words_create accepts it -> `out` with the separator's default filled in.
static int check_spec(const kgpu_words_spec *spec, const char *who, kgpu_words_spec &out) {
    if (!spec) { set_error("%s: null spec", who); return KGPU_ERR_INVALID_ARG; }
    if (spec->size < sizeof(kgpu_words_spec)) { set_error("%s: spec.size %u, the struct has %zu bytes", who, spec->size, sizeof(kgpu_words_spec)); return KGPU_ERR_INVALID_ARG; }
    out = *spec;
    if (out.field < KGPU_WORDS_SURFACE) { set_error("%s: field %d (KGPU_WORDS_SURFACE, or a feature index from 0)", who, out.field); return KGPU_ERR_INVALID_ARG; }
    if (out.filter > KGPU_WORDS_KEEP) { set_error("%s: unknown filter %u", who, out.filter); return KGPU_ERR_INVALID_ARG; }
    if (out.separator > 255 || out.separator == '\n') { set_error("%s: separator %u (one byte, not '\\n')", who, out.separator); return KGPU_ERR_INVALID_ARG; }
    if (out.separator == 0) out.separator = ' ';
    if (out.n_names) {
        if (!out.name_offsets) { set_error("%s: names without offsets", who); return KGPU_ERR_INVALID_ARG; }
        for (uint64_t i = 0; i < out.n_names; ++i)
            if (out.name_offsets[i + 1] < out.name_offsets[i]) { set_error("%s: name offsets run backwards at %llu", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
        if (out.name_offsets[out.n_names] != out.name_offsets[0] && !out.names) { set_error("%s: name offsets without names", who); return KGPU_ERR_INVALID_ARG; }
    }
    return KGPU_OK;
}

extern "C" int kgpu_words_create(kgpu_dict *d, const kgpu_words_spec *spec, kgpu_words **out) {
    const char *who = "kgpu_words_create";
    if (!d || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    kgpu_words_spec sp;
    int rc;
    if ((rc = check_spec(spec, who, sp)) || (rc = require_features(d, who))) return rc;
    std::vector<WordRow> rows;
    std::vector<uint8_t> names;
    // (kgpu_dict_set_features writes the blobs once, in the same feat_mu critical section that sets d->feat, and never again: require_features
    // has taken that lock and seen d->feat, so they are complete and read here without it -- handles of one dictionary are made side by side)
    if ((rc = build_word_table(d->feat_blob_known.data(), d->feat_blob_known.size(), d->feat_blob_unk.data(), d->feat_blob_unk.size(),
                               d->info.n_morphs, d->info.n_unk_morphs, sp, rows, names)))
        return rc;
    HIPCHECK(hipSetDevice(d->device));
    void *dr = nullptr, *dn = nullptr;
    const size_t row_bytes = std::max<size_t>(rows.size() * sizeof(WordRow), 16), name_bytes = std::max<size_t>(names.size(), 16);
    HIPCHECK(hipMalloc(&dr, row_bytes));
    if (hipMalloc(&dn, name_bytes) != hipSuccess) { (void)hipFree(dr); set_error("%s: hipMalloc of %zu bytes failed", who, name_bytes); return KGPU_ERR_HIP; }
    if ((!rows.empty() && hipMemcpy(dr, rows.data(), rows.size() * sizeof(WordRow), hipMemcpyHostToDevice) != hipSuccess) ||
        (!names.empty() && hipMemcpy(dn, names.data(), names.size(), hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(dr); (void)hipFree(dn);
        set_error("%s: upload of the word table failed", who);
        return KGPU_ERR_HIP;
    }
    kgpu_words *w = new kgpu_words();
    w->dict = d;
    d->refs.fetch_add(1, std::memory_order_relaxed);
    w->field = sp.field; w->filter = sp.filter; w->sep = sp.separator;
    w->d_rows = dr; w->d_names = dn;
    w->h_rows = std::move(rows); w->h_names = std::move(names);
    *out = w;
    return KGPU_OK;
}

extern "C" void kgpu_words_destroy(kgpu_words *w) {
    if (w) words_release(w);
}

void kgpu::words_release(kgpu_words *w) {
    if (w->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;   // a counts handle still reads the tables
    kgpu_dict *d = w->dict;
    (void)hipSetDevice(d->device);
    (void)hipFree(w->d_rows);
    (void)hipFree(w->d_names);
    delete w;
    if (d->closed.load(std::memory_order_acquire)) {   // the caller's dictionary handle is gone: the contexts this handle's calls pooled go with it
        std::vector<kgpu_ctx *> pooled;
        {
            std::lock_guard<std::mutex> g(d->pool_mu);
            pooled.swap(d->pool);
        }
        for (auto *c : pooled) kgpu_ctx_destroy(c);
    }
    dict_release(d);
}

WordTable kgpu::word_table(const kgpu_words *w) {
    return WordTable{(const WordRow *)w->d_rows, (const uint8_t *)w->d_names, w->sep, w->filter == KGPU_WORDS_KEEP};
}

int kgpu::enqueue_words(kgpu_ctx *c, const kgpu_words *w, const DeviceRecords &r, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, const char *who) {
    if (w->dict != c->dict) { set_error("%s: the context's dictionary is not the words handle's", who); return KGPU_ERR_INVALID_ARG; }
    WordsArgs a{};
    if (int rc = records_batch(c, r, (size_t)r.n * 8 + 8, d_text_offsets, a.b)) return rc;
    a.w = word_table(w);
    a.text = d_text; a.text_cap = text_capacity;
    return records_launched(c, launch_format_words(a, c->stream), who, "render", text_capacity);
}

extern "C" int kgpu_format_words_device(kgpu_ctx *c, const kgpu_words *w, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                        const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                                        uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets) {
    const char *who = "kgpu_format_words_device";
    if (!c || !w || !d_offsets || !d_tok_offsets || !d_text_offsets || (n && (!d_utf8 || !d_tokens)) || (text_capacity && !d_text)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (w->dict != c->dict) { set_error("%s: the context's dictionary is not the words handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_words(c, w, DeviceRecords{d_utf8, d_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, d_text, text_capacity, d_text_offsets, who);
}

// Test hook (host only, not in the header): the spec check and the word table of kgpu_words_create without a device or a handle.
// entries: (n_morphs + n_unk) x 2 uint32 -- offset into the pool, then length | 1 << 30 (the word is the surface) | 1 << 31 (dropped).
// *separator: the byte the handle would use.  KGPU_ERR_CAPACITY: pool_cap < *pool_len (the entries are written all the same).
extern "C" int kgpu_debug_word_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                                     const kgpu_words_spec *spec, uint32_t *entries, uint8_t *pool, uint64_t pool_cap, uint64_t *pool_len, uint32_t *separator) {
    kgpu_words_spec sp;
    int rc;
    if ((rc = check_spec(spec, "kgpu_debug_word_table", sp))) return rc;
    std::vector<WordRow> rows;
    std::vector<uint8_t> names;
    if ((rc = build_word_table(known, known_len, unk, unk_len, n_morphs, n_unk, sp, rows, names))) return rc;
    if (separator) *separator = sp.separator;
    if (pool_len) *pool_len = names.size();
    if (entries && !rows.empty()) std::memcpy(entries, rows.data(), rows.size() * sizeof(WordRow));
    if (names.size() > pool_cap) { set_error("pool buffer too small: need %zu", names.size()); return KGPU_ERR_CAPACITY; }
    if (!names.empty()) std::memcpy(pool, names.data(), names.size());
    return KGPU_OK;
}
