// kanpyo_amd/csrc/kgpu_decode_device.cpp -- the text from ids (include/kanpyo_gpu.h, "text from ids"; kgpu_decode.hip) behind the C ABI: kgpu_decode_device,
// enqueued on a context as a render is (the context's lines_report and lines_len, waited for by kgpu_ctx_sync_lines, which reports the bytes), and
// kgpu_decode_batch, the host form -- per chunk of sequences one upload, one enqueue, one sync, one download on a pooled context, chunk after chunk:
// the simple route, not a pipeline.  The arguments are checked by kgpu_decode_host.cpp's decode_check_args, which kgpu_decode_host shares.
//
// The id -> arena entry table (4 bytes per list entry; build_decode_entries made it when the handle was created) goes to the device with the handle's
// FIRST decode call, under the handle's own lock: a handle that never decodes holds what it held before.
#include <algorithm>

#include "kgpu_runtime.h"

namespace {

int ensure_decode_table(const kgpu_vocab *v, const char *who) {
    std::lock_guard<std::mutex> g(v->decode_mu);
    if (v->d_entry) return KGPU_OK;
    void *p = nullptr;
    const size_t bytes = v->h_entry.size() * 4;
    if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess || (bytes && hipMemcpy(p, v->h_entry.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        set_error("%s: no device memory for, or no upload of, the id -> word table: %zu bytes", who, bytes);
        return KGPU_ERR_HIP;
    }
    v->d_entry = p;
    std::vector<uint32_t>().swap(v->h_entry);   // (the device copy is the one that is read from now on)
    return KGPU_OK;
}

// The enqueue on c's stream behind whatever is queued there; the arguments are checked.
int enqueue_decode(kgpu_ctx *c, const kgpu_vocab *v, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *opts,
                   uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status, const char *who) {
    int rc;
    if ((rc = ensure_decode_table(v, who))) return rc;
    DecodeArgs a{};
    // (of the renders' batch the scan uses n, the scratch, the mirror and the host's words; there are no records and no text here)
    if ((rc = records_batch(c, DeviceRecords{nullptr, nullptr, n, nullptr, nullptr, nullptr, nullptr}, (size_t)n * 8 + 8, d_text_offsets, a.b))) return rc;
    a.r = decode_rule(opts, v->prefix, v->prefix_len, v->n_words);
    a.ids = d_ids; a.id_offsets = d_id_offsets; a.width = width;
    a.entry = (const uint32_t *)v->d_entry; a.arena = (const uint8_t *)v->d_arena;
    a.status = d_status; a.text = d_text; a.text_cap = text_capacity;
    return records_launched(c, launch_decode(a, c->stream), who, "decode", text_capacity);
}

}  // namespace

extern "C" int kgpu_decode_device(kgpu_ctx *c, const kgpu_vocab *v, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, uint64_t width,
                                  const kgpu_decode_opts *opts, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status) {
    const char *who = "kgpu_decode_device";
    if (!c || !v) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = decode_check_args(who, d_ids, d_id_offsets, false, n, width, opts, v->prefix_len, d_text, text_capacity, d_text_offsets, d_status))) return rc;
    if (v->words->dict != c->dict) { set_error("%s: the context's dictionary is not the vocabulary handle's", who); return KGPU_ERR_INVALID_ARG; }
    if ((rc = begin_records_call(c, who))) return rc;
    return enqueue_decode(c, v, d_ids, d_id_offsets, n, width, opts, d_text, text_capacity, d_text_offsets, d_status, who);
}

extern "C" int kgpu_decode_batch(kgpu_vocab *v, const int32_t *ids, const uint64_t *id_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *opts,
                                 uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    const char *who = "kgpu_decode_batch";
    if (n_bytes) *n_bytes = 0;
    if (!v) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = decode_check_args(who, ids, id_offsets, true, n, width, opts, v->prefix_len, text, text_capacity, text_offsets, status))) return rc;
    kgpu_dict *d = v->words->dict;
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    kgpu_ctx *c = lease.c;
    if ((rc = lease.rc)) return rc;
    const uint64_t max_seqs = std::max<uint64_t>(1, test_hooks().chunk_sents), max_ids = 4ull << 20;
    const auto first_id = [&](uint64_t s) { return id_offsets ? id_offsets[s] : s * width; };
    uint64_t done = 0, total = 0;   // sequences delivered, their bytes
    bool overflow = false;          // a chunk did not fit what was left of `text`: the chunks behind it are only measured
    text_offsets[0] = 0;
    while (done < n) {
        uint64_t m = 1;
        while (done + m < n && m < max_seqs && first_id(done + m + 1) - first_id(done) <= max_ids) ++m;
        const uint64_t i0 = first_id(done), n_ids = first_id(done + m) - i0;
        if ((rc = c->out_tok.ensure((size_t)n_ids * 4 + 16)) || (rc = c->in_off.ensure(((size_t)m + 1) * 8)) || (rc = c->out_off.ensure(((size_t)m + 1) * 8)) ||
            (rc = c->out_status.ensure((size_t)m + 16))) return rc;
        if (n_ids && (rc = ctx_h2d(c, c->out_tok.p, ids + i0, (size_t)n_ids * 4, "H2D ids"))) return rc;
        if (id_offsets && (rc = ctx_h2d(c, c->in_off.p, id_offsets + done, ((size_t)m + 1) * 8, "H2D id offsets"))) return rc;
        // (the offsets are as the caller has them: the ids are biased by the chunk's first; a padded chunk's rows start at 0)
        const int32_t *d_ids = (const int32_t *)c->out_tok.p - (id_offsets ? i0 : 0);
        const uint64_t left = overflow ? 0 : text_capacity - total;
        uint64_t room = std::min<uint64_t>(left, std::max<uint64_t>(4096, n_ids * 16)), need = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {   // (a chunk longer than the guess and no longer than what is left: once more, at its size)
            if ((rc = c->norm_text.ensure((size_t)room + 16))) return rc;
            if ((rc = enqueue_decode(c, v, d_ids, id_offsets ? (const uint64_t *)c->in_off.p : nullptr, m, width, opts, (uint8_t *)c->norm_text.p, room,
                                     (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p, who))) return rc;
            rc = kgpu_ctx_sync_lines(c, &need);
            if (rc != KGPU_ERR_CAPACITY || need > left) break;
            room = need;
        }
        if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
        if (rc == KGPU_ERR_CAPACITY) overflow = true;
        else if (need && hipMemcpy(text + total, c->norm_text.p, (size_t)need, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H text failed", who); return KGPU_ERR_HIP; }
        if (hipMemcpy(text_offsets + done, c->out_off.p, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H offsets failed", who); return KGPU_ERR_HIP; }
        if (hipMemcpy(status + done, c->out_status.p, (size_t)m, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H status failed", who); return KGPU_ERR_HIP; }
        for (uint64_t s = done; s <= done + m; ++s) text_offsets[s] += total;   // chunk-relative -> the call's
        total += need;
        done += m;
    }
    if (n_bytes) *n_bytes = total;
    if (overflow) {
        set_error("%s: text buffer too small: need %llu, capacity %llu", who, (unsigned long long)total, (unsigned long long)text_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}
