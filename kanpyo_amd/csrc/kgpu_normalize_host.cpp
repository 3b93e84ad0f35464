// kanpyo_amd/csrc/kgpu_normalize_host.cpp -- NFC / NFKC on the device (kgpu_normalize.hip) behind the C ABI (include/kanpyo_gpu.h, "text normalisation").
//
// Owns: the upload of the tables (kgpu_normalize_table.cpp holds them; once per dictionary handle), kgpu_normalize_device / kgpu_ctx_sync_normalize (a batch
// resident in HBM, on a context's stream, reported through the context's lines_report as a render is), and the two host forms: kgpu_normalize_batch (packed
// lines: one copy to the device, the three launches, the results back) and kgpu_normalize_text (a raw block: split_block first, the normaliser reads the
// split's output where it lies).  Each host call is one batch on one pooled context: the normaliser moves a byte or two per input byte.
// The `_aligned` twins of all of them (include/kanpyo_gpu.h, "source alignment") are the same calls with the edit records beside the text: the context's
// report then carries two sizes.  kgpu_source_spans_device / _batch (kgpu_align.hip) map token records through such edits.
#include <vector>

#include "kgpu_runtime.h"

static bool known_form(int form) { return form == KGPU_NORMALIZE_NFC || form == KGPU_NORMALIZE_NFKC; }

static int ensure_norm_tables(kgpu_dict *d) {
    std::lock_guard<std::mutex> g(d->feat_mu);   // (the lock of everything a handle uploads after its creation: allocs and device_bytes change under it)
    if (d->norm_ready) return KGPU_OK;
    const NormTables h = norm_host_tables();
    const NormTableSizes z = norm_table_sizes();
    const void *src[6] = {h.stage1, h.stage2, h.dec, h.pool, h.comp_key, h.comp_val};
    const size_t bytes[6] = {z.stage1, z.stage2, z.dec, z.pool, z.comp_key, z.comp_val};
    size_t at[6], total = 0;
    for (int k = 0; k < 6; ++k) { at[k] = total; total += (bytes[k] + 15) & ~(size_t)15; }
    uint8_t *p = nullptr;
    HIPCHECK(hipMalloc((void **)&p, total));
    for (int k = 0; k < 6; ++k)
        if (hipMemcpy(p + at[k], src[k], bytes[k], hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); set_error("upload of the normaliser's tables failed"); return KGPU_ERR_HIP; }
    d->allocs.push_back(p);   // (recorded once it is whole: a failed upload leaves nothing behind)
    d->info.device_bytes += total;
    d->norm = NormTables{(const uint16_t *)(p + at[0]), (const uint32_t *)(p + at[1]), (const uint32_t *)(p + at[2]), (const uint32_t *)(p + at[3]),
                         (const uint64_t *)(p + at[4]), (const uint32_t *)(p + at[5]), h.n_comp};
    d->norm_ready = true;
    return KGPU_OK;
}

int kgpu::enqueue_normalize(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint8_t *d_text, uint64_t text_capacity,
                            uint64_t *d_text_offsets, uint8_t *d_status, const char *who) {
    int rc;
    if ((rc = ensure_norm_tables(c->dict)) || (rc = c->lines_report.arm()) || (rc = c->lines_len.ensure(((size_t)n + 1) * 8 + (size_t)n + 16))) return rc;
    NormArgs a{};
    a.t = c->dict->norm; a.form = (uint32_t)form;
    a.utf8 = d_utf8; a.offsets = d_offsets; a.n = n;
    a.sent_len = (uint64_t *)c->lines_len.p; a.mode = (uint8_t *)c->lines_len.p + ((size_t)n + 1) * 8;
    a.text_offsets = d_text_offsets; a.status = d_status;
    a.text = d_text; a.text_cap = text_capacity;
    a.host_ctl = c->lines_report.dev();
    return records_launched(c, launch_normalize(a, c->stream), who, "normalise", text_capacity);
}

int kgpu::enqueue_normalize_aligned(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint8_t *d_text, uint64_t text_capacity,
                                    uint64_t *d_text_offsets, uint8_t *d_status, kgpu_norm_edit *d_edits, uint64_t edit_capacity, uint64_t *d_edit_offsets, const char *who) {
    int rc;
    if ((rc = ensure_norm_tables(c->dict)) || (rc = c->lines_report.arm()) || (rc = c->lines_len.ensure(((size_t)n + 1) * 16 + (size_t)n + 16))) return rc;
    NormAlignArgs a{};
    a.t = c->dict->norm; a.form = (uint32_t)form;
    a.utf8 = d_utf8; a.offsets = d_offsets; a.n = n;
    a.sent_len = (uint64_t *)c->lines_len.p; a.edit_len = a.sent_len + n + 1; a.mode = (uint8_t *)(a.edit_len + n + 1);
    a.text_offsets = d_text_offsets; a.status = d_status;
    a.text = d_text; a.text_cap = text_capacity;
    a.edit_offsets = d_edit_offsets; a.edits = d_edits; a.edit_cap = edit_capacity;
    a.host_ctl = c->lines_report.dev();
    if ((rc = records_launched(c, launch_normalize_aligned(a, c->stream), who, "normalise", text_capacity))) return rc;
    c->lines_report.two_sizes = true; c->lines_report.cap1 = edit_capacity;
    return KGPU_OK;
}

static int check_normalize_device(const char *who, kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint8_t *d_text, uint64_t text_capacity,
                                  uint64_t *d_text_offsets, uint8_t *d_status) {
    if (!c || !d_offsets || !d_text_offsets || (n && (!d_utf8 || !d_status)) || (text_capacity && !d_text)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (!known_form(form)) { set_error("%s: unknown form %d", who, form); return KGPU_ERR_INVALID_ARG; }
    if (d_text && d_utf8 && d_utf8 >= d_text && (d_utf8 == d_text || d_utf8 < d_text + text_capacity)) { set_error("%s: d_text overlaps d_utf8", who); return KGPU_ERR_INVALID_ARG; }
    return KGPU_OK;
}

extern "C" int kgpu_normalize_device_aligned(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                             uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status,
                                             kgpu_norm_edit *d_edits, uint64_t edit_capacity, uint64_t *d_edit_offsets) {
    const char *who = "kgpu_normalize_device_aligned";
    if (int rc = check_normalize_device(who, c, form, d_utf8, d_offsets, n, d_text, text_capacity, d_text_offsets, d_status)) return rc;
    if (!d_edit_offsets || (edit_capacity && !d_edits)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_normalize_aligned(c, form, d_utf8, d_offsets, n, d_text, text_capacity, d_text_offsets, d_status, d_edits, edit_capacity, d_edit_offsets, who);
}

extern "C" int kgpu_ctx_sync_normalize_aligned(kgpu_ctx *c, uint64_t *n_bytes, uint64_t *n_edits) {
    if (!c) { set_error("kgpu_ctx_sync_normalize_aligned: null ctx"); return KGPU_ERR_INVALID_ARG; }
    if (n_edits) *n_edits = 0;
    const bool aligned = c->lines_report.pending && c->lines_report.two_sizes;
    const int rc = kgpu_ctx_sync_lines(c, n_bytes);   // (the report carries two sizes: [0] bytes, [1] edits)
    if (aligned && n_edits && (rc == KGPU_OK || rc == KGPU_ERR_CAPACITY)) *n_edits = c->lines_report.word1;
    return rc;
}

extern "C" int kgpu_normalize_device(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                     uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status) {
    const char *who = "kgpu_normalize_device";
    if (int rc = check_normalize_device(who, c, form, d_utf8, d_offsets, n, d_text, text_capacity, d_text_offsets, d_status)) return rc;
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_normalize(c, form, d_utf8, d_offsets, n, d_text, text_capacity, d_text_offsets, d_status, who);
}

extern "C" int kgpu_ctx_sync_normalize(kgpu_ctx *c, uint64_t *n_bytes) {
    if (!c) { set_error("kgpu_ctx_sync_normalize: null ctx"); return KGPU_ERR_INVALID_ARG; }
    return kgpu_ctx_sync_lines(c, n_bytes);   // (the normaliser reports as a render does: [0] bytes, [1] stays 0)
}

// The lines in device memory (d_in, d_off: n + 1 offsets; `total` bytes) normalised on c into c->norm_text, and the results into the caller's host arrays.
// lines_short: the caller's offsets table cannot hold the lines (the sizes are still found).  *n_bytes: the exact size.
// al (may be null): the aligned forms' edit buffers; *al->n_edits: the exact number of records.
struct AlignedOut { kgpu_norm_edit *edits; uint64_t edit_capacity; uint64_t *edit_offsets; uint64_t *n_edits; };
static int normalize_to_host(kgpu_ctx *c, int form, const uint8_t *d_in, const uint64_t *d_off, uint64_t n, uint64_t total, uint8_t *text, uint64_t text_capacity,
                             uint64_t *text_offsets, uint8_t *status, bool lines_short, uint64_t *n_bytes, const char *who, const AlignedOut *al = nullptr) {
    int rc;
    const uint64_t bound = total * NORM_MAX_EXPANSION, room = text_capacity < bound ? text_capacity : bound;
    if ((rc = c->norm_text.ensure((size_t)room + 16)) || (rc = c->out_off.ensure(((size_t)n + 1) * 8)) || (rc = c->out_status.ensure((size_t)n + 16))) return rc;
    uint64_t need = 0, need_edits = 0;
    if (al) {   // (an edit covers a source byte at least: `total` records always suffice)
        const uint64_t eroom = al->edit_capacity < total ? al->edit_capacity : total;
        if ((rc = c->norm_edits.ensure((size_t)eroom * sizeof(kgpu_norm_edit) + 16)) || (rc = c->norm_eoff.ensure(((size_t)n + 1) * 8))) return rc;
        if ((rc = enqueue_normalize_aligned(c, form, d_in, d_off, n, (uint8_t *)c->norm_text.p, room, (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p,
                                            (kgpu_norm_edit *)c->norm_edits.p, eroom, (uint64_t *)c->norm_eoff.p, who))) return rc;
        rc = kgpu_ctx_sync_normalize_aligned(c, &need, &need_edits);
        *al->n_edits = need_edits;
    } else {
        if ((rc = enqueue_normalize(c, form, d_in, d_off, n, (uint8_t *)c->norm_text.p, room, (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p, who))) return rc;
        rc = kgpu_ctx_sync_normalize(c, &need);
    }
    *n_bytes = need;
    if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    if (rc == KGPU_ERR_CAPACITY || lines_short) {
        if (al) set_error("%s: buffers too small: need %llu text bytes (capacity %llu), %llu edit records (capacity %llu) and %llu offsets", who, (unsigned long long)need,
                          (unsigned long long)text_capacity, (unsigned long long)need_edits, (unsigned long long)al->edit_capacity, (unsigned long long)(n + 1));
        else set_error("%s: buffers too small: need %llu text bytes (capacity %llu) and %llu offsets", who, (unsigned long long)need, (unsigned long long)text_capacity,
                       (unsigned long long)(n + 1));
        return KGPU_ERR_CAPACITY;
    }
    if (al) {
        if (need_edits && hipMemcpy(al->edits, c->norm_edits.p, (size_t)need_edits * sizeof(kgpu_norm_edit), hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H edits failed", who); return KGPU_ERR_HIP; }
        if (hipMemcpy(al->edit_offsets, c->norm_eoff.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H edit offsets failed", who); return KGPU_ERR_HIP; }
    }
    if (need && hipMemcpy(text, c->norm_text.p, (size_t)need, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H text failed", who); return KGPU_ERR_HIP; }
    if (hipMemcpy(text_offsets, c->out_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H offsets failed", who); return KGPU_ERR_HIP; }
    if (status && n && hipMemcpy(status, c->out_status.p, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H status failed", who); return KGPU_ERR_HIP; }
    return KGPU_OK;
}

static bool aligned_args_ok(const AlignedOut *al, bool offsets_needed) {
    if (!al) return true;
    if (al->n_edits) *al->n_edits = 0;
    return al->n_edits && (!offsets_needed || al->edit_offsets) && (!al->edit_capacity || al->edits);
}

static int normalize_batch(const char *who, kgpu_dict *d, int form, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                           uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes, const AlignedOut *al) {
    if (!d || !offsets || !text_offsets || !n_bytes || (text_capacity && !text) || !aligned_args_ok(al, true)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *n_bytes = 0;
    if (!known_form(form)) { set_error("%s: unknown form %d", who, form); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = check_host_batch(who, offsets, n, utf8))) return rc;
    const uint64_t total = offsets[n] - offsets[0];
    if (total >= (1ull << 32)) { set_error("%s: 4 GiB of text or more; split the batch", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    kgpu_ctx *c = lease.c;
    if ((rc = lease.rc) || (rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure(((size_t)n + 1) * 8))) return rc;
    if (total && (rc = ctx_h2d(c, c->in_utf8.p, utf8 + offsets[0], (size_t)total, "H2D text"))) return rc;
    if ((rc = ctx_h2d(c, c->in_off.p, offsets, ((size_t)n + 1) * 8, "H2D offsets"))) return rc;
    const uint8_t *d_in = (const uint8_t *)c->in_utf8.p - offsets[0];   // (the offsets are as the caller has them)
    return normalize_to_host(c, form, d_in, (const uint64_t *)c->in_off.p, n, total, text, text_capacity, text_offsets, status, false, n_bytes, who, al);
}

extern "C" int kgpu_normalize_batch(kgpu_dict *d, int form, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                    uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    return normalize_batch("kgpu_normalize_batch", d, form, utf8, offsets, n, text, text_capacity, text_offsets, status, n_bytes, nullptr);
}
extern "C" int kgpu_normalize_batch_aligned(kgpu_dict *d, int form, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                            uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes,
                                            kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *edit_offsets, uint64_t *n_edits) {
    const AlignedOut al{edits, edit_capacity, edit_offsets, n_edits};
    return normalize_batch("kgpu_normalize_batch_aligned", d, form, utf8, offsets, n, text, text_capacity, text_offsets, status, n_bytes, &al);
}

static int normalize_text(const char *who, kgpu_dict *d, int form, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                          uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes, const AlignedOut *al) {
    if (!d || (len && !text) || (text_capacity && !out_text) || (offsets_capacity && !text_offsets) || !n_lines || !n_bytes || !aligned_args_ok(al, offsets_capacity != 0)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *n_lines = 0; *n_bytes = 0;
    if (!known_form(form)) { set_error("%s: unknown form %d", who, form); return KGPU_ERR_INVALID_ARG; }
    if (len >= (1ull << 32)) { set_error("%s: block of 4 GiB or more; split it", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(d->device));
    int rc;
    PooledCtx lease(d);
    kgpu_ctx *c = lease.c;
    std::vector<uint64_t> off;
    uint64_t lines = 0;
    if ((rc = lease.rc) || (rc = split_block(c, text, len, who, off, lines))) return rc;
    *n_lines = lines;
    return normalize_to_host(c, form, (const uint8_t *)c->split_text.p, (const uint64_t *)c->split_off.p, lines, off[lines], out_text, text_capacity,
                             text_offsets, status, lines + 1 > offsets_capacity, n_bytes, who, al);
}

extern "C" int kgpu_normalize_text(kgpu_dict *d, int form, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                                   uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    return normalize_text("kgpu_normalize_text", d, form, text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes, nullptr);
}
extern "C" int kgpu_normalize_text_aligned(kgpu_dict *d, int form, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                                           uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes,
                                           kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *edit_offsets, uint64_t *n_edits) {
    const AlignedOut al{edits, edit_capacity, edit_offsets, n_edits};
    return normalize_text("kgpu_normalize_text_aligned", d, form, text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes, &al);
}

// ------------------------------------------------------- source spans of token records (kgpu_align.hip)
static int enqueue_source_spans(kgpu_ctx *c, const kgpu_token *d_tokens, const uint64_t *d_tok_offsets, uint64_t n, const kgpu_norm_edit *d_edits,
                                const uint64_t *d_edit_offsets, kgpu_span *d_spans, uint64_t span_capacity, const char *who) {
    SpansArgs a{};
    // (the walk of the renders reads a sentence's text length beside its records; nothing here looks at text: the token offsets stand in for the text's)
    if (int rc = records_batch(c, DeviceRecords{nullptr, d_tok_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, 16, nullptr, a.b)) return rc;
    a.edits = d_edits; a.edit_offsets = d_edit_offsets; a.spans = d_spans; a.span_cap = span_capacity;
    return records_launched(c, launch_source_spans(a, c->stream), who, "span", ~0ull);
}

extern "C" int kgpu_source_spans_device(kgpu_ctx *c, const kgpu_token *d_tokens, const uint64_t *d_tok_offsets, uint64_t n,
                                        const kgpu_norm_edit *d_edits, const uint64_t *d_edit_offsets, kgpu_span *d_spans, uint64_t span_capacity) {
    const char *who = "kgpu_source_spans_device";
    if (!c || !d_tok_offsets || !d_edit_offsets || (span_capacity && (!d_spans || !d_tokens))) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_spans & 15u) { set_error("%s: d_spans is not 16-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_source_spans(c, d_tokens, d_tok_offsets, n, d_edits, d_edit_offsets, d_spans, span_capacity, who);
}

extern "C" int kgpu_source_spans_batch(kgpu_dict *d, const kgpu_token *tokens, const uint64_t *tok_offsets, uint64_t n, const kgpu_norm_edit *edits,
                                       const uint64_t *edit_offsets, kgpu_span *spans) {
    const char *who = "kgpu_source_spans_batch";
    if (!d || !tok_offsets || !edit_offsets) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n; ++i)
        if (tok_offsets[i + 1] < tok_offsets[i] || edit_offsets[i + 1] < edit_offsets[i]) { set_error("%s: offsets run backwards at sentence %llu", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    const uint64_t t0 = tok_offsets[0], nt = tok_offsets[n] - t0, e0 = edit_offsets[0], ne = edit_offsets[n] - e0;
    if ((nt && (!tokens || !spans)) || (ne && !edits)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (!nt) return KGPU_OK;
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    kgpu_ctx *c = lease.c;
    int rc;
    if ((rc = lease.rc) || (rc = c->out_tok.ensure((size_t)nt * sizeof(kgpu_token))) || (rc = c->out_off.ensure(((size_t)n + 1) * 8)) ||
        (rc = c->norm_edits.ensure((size_t)ne * sizeof(kgpu_norm_edit) + 16)) || (rc = c->norm_eoff.ensure(((size_t)n + 1) * 8)) || (rc = c->span_out.ensure((size_t)nt * sizeof(kgpu_span)))) return rc;
    if ((rc = ctx_h2d(c, c->out_tok.p, tokens + t0, (size_t)nt * sizeof(kgpu_token), "H2D tokens")) || (rc = ctx_h2d(c, c->out_off.p, tok_offsets, ((size_t)n + 1) * 8, "H2D token offsets")) ||
        (ne && (rc = ctx_h2d(c, c->norm_edits.p, edits + e0, (size_t)ne * sizeof(kgpu_norm_edit), "H2D edits"))) || (rc = ctx_h2d(c, c->norm_eoff.p, edit_offsets, ((size_t)n + 1) * 8, "H2D edit offsets"))) return rc;
    // (the offsets are as the caller has them: the three arrays are biased by their first entries)
    if ((rc = enqueue_source_spans(c, (const kgpu_token *)c->out_tok.p - t0, (const uint64_t *)c->out_off.p, n, (const kgpu_norm_edit *)c->norm_edits.p - e0,
                                   (const uint64_t *)c->norm_eoff.p, (kgpu_span *)c->span_out.p - t0, t0 + nt, who))) return rc;
    if ((rc = kgpu_ctx_sync_lines(c, nullptr))) return rc;
    if (hipMemcpy(spans, c->span_out.p, (size_t)nt * sizeof(kgpu_span), hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H spans failed", who); return KGPU_ERR_HIP; }
    return KGPU_OK;
}
