// kanpyo_amd/csrc/kgpu_sentence_batch.cpp -- lines cut into sentences on the device (kgpu_sentence.hip) behind the C ABI (include/kanpyo_gpu.h, "sentences").
//
// Owns: kgpu_split_sentences_device / kgpu_ctx_sync_sentences (a batch resident in HBM, on a context's stream, reported through the context's lines_report
// as a normalise is: two sizes, the sentences -- compared with the capacity -- and their bytes), and kgpu_split_sentences_batch (packed lines in host
// memory: chunks cut at line ends, one after the other on one pooled context; a chunk's offsets and line numbers are made the call's on the host).
#include <vector>

#include "kgpu_runtime.h"

static int enqueue_sentences(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total, const SentRule &rule, uint8_t *d_out,
                             uint64_t *d_out_offsets, kgpu_sentence *d_sents, uint64_t sent_capacity, const char *who) {
    SentArgs a{};
    a.utf8 = d_utf8; a.offsets = d_offsets; a.n = n; a.total = total; a.rule = rule;
    a.out = d_out; a.out_offsets = d_out_offsets; a.sents = d_sents; a.sent_cap = sent_capacity;
    a.ntiles = sent_tiles(total);
    int rc;
    if ((rc = c->lines_report.arm()) || (rc = c->lines_len.ensure(sent_scratch_bytes(a.ntiles)))) return rc;
    sent_place_scratch(a, c->lines_len.p);
    a.host_ctl = c->lines_report.dev();
    if ((rc = records_launched(c, launch_split_sentences(a, c->stream), who, "sentence split", sent_capacity))) return rc;
    c->lines_report.two_sizes = true; c->lines_report.cap1 = ~0ull;   // (word [1], the bytes, is a size that always fits)
    return KGPU_OK;
}

extern "C" int kgpu_split_sentences_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                                           const kgpu_sentence_opts *opts, uint8_t *d_out, uint64_t *d_out_offsets, kgpu_sentence *d_sents, uint64_t sent_capacity) {
    const char *who = "kgpu_split_sentences_device";
    if (!c || !d_offsets || !d_out_offsets || (total_bytes && (!d_utf8 || !d_out)) || (sent_capacity && !d_sents)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    SentRule rule;
    if (int rc = sent_rule_from_opts(who, opts, rule)) return rc;
    if (total_bytes >= (1ull << 32)) { set_error("%s: 4 GiB of text or more; split the batch", who); return KGPU_ERR_INVALID_ARG; }
    if (!n && total_bytes) { set_error("%s: %llu bytes of text in no lines", who, (unsigned long long)total_bytes); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)d_sents & 15u) { set_error("%s: d_sents is not 16-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if (total_bytes && d_utf8 >= d_out && d_utf8 < d_out + total_bytes) { set_error("%s: d_out overlaps d_utf8", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_sentences(c, d_utf8, d_offsets, n, total_bytes, rule, d_out, d_out_offsets, d_sents, sent_capacity, who);
}

extern "C" int kgpu_ctx_sync_sentences(kgpu_ctx *c, uint64_t *n_sentences, uint64_t *n_bytes) {
    if (!c) { set_error("kgpu_ctx_sync_sentences: null ctx"); return KGPU_ERR_INVALID_ARG; }
    if (n_sentences) *n_sentences = 0;
    if (n_bytes) *n_bytes = 0;
    if (!c->lines_report.pending) return KGPU_OK;
    const uint64_t cap = c->lines_report.cap;
    uint64_t S = 0;
    const int rc = kgpu_ctx_sync_lines(c, &S);   // (the report carries two sizes: [0] sentences, [1] bytes)
    if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    if (n_sentences) *n_sentences = S;
    if (rc == KGPU_ERR_CAPACITY) { set_error("kgpu_ctx_sync_sentences: %llu sentences, capacity %llu", (unsigned long long)S, (unsigned long long)cap); return rc; }
    if (n_bytes) *n_bytes = c->lines_report.word1;
    return KGPU_OK;
}

extern "C" int kgpu_split_sentences_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_sentence_opts *opts, uint8_t *out,
                                          uint64_t *out_offsets, kgpu_sentence *sents, uint64_t sent_capacity, uint64_t *n_sentences) {
    const char *who = "kgpu_split_sentences_batch";
    if (n_sentences) *n_sentences = 0;
    if (!d || !offsets || !out_offsets || !n_sentences || (sent_capacity && !sents)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    SentRule rule;
    int rc;
    if ((rc = sent_rule_from_opts(who, opts, rule)) || (rc = check_host_batch(who, offsets, n, utf8))) return rc;
    const uint64_t total = offsets[n] - offsets[0];
    if (total >= (1ull << 32)) { set_error("%s: 4 GiB of text or more; split the batch", who); return KGPU_ERR_INVALID_ARG; }
    if (total && !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    kgpu_ctx *c = lease.c;
    if ((rc = lease.rc)) return rc;
    // chunks of 64 MiB and a million lines (the kernels are dealt bytes: a chunk costs five launches whatever it holds); the test hooks make them small
    const TestHooks hooks = test_hooks();
    const uint64_t max_bytes = hooks.chunk_bytes == TestHooks().chunk_bytes ? 64ull << 20 : hooks.chunk_bytes;
    const uint64_t max_lines = hooks.chunk_sents == TestHooks().chunk_sents ? 1ull << 20 : hooks.chunk_sents;
    std::vector<uint64_t> rel;
    uint64_t S = 0, at = 0;   // sentences and bytes delivered (S goes on counting once they no longer fit)
    bool overflow = false;
    for (uint64_t lo = 0; lo < n || (n == 0 && lo == 0);) {
        const uint64_t m = n ? cut_chunk(offsets, lo, n, max_lines, max_bytes) : 0, bytes = offsets[lo + m] - offsets[lo];
        const uint64_t bound = bytes + m, room = overflow ? 0 : sent_capacity - S, cap = room < bound ? room : bound;   // (a sentence behind a line's first holds a terminator)
        if ((rc = c->in_utf8.ensure((size_t)bytes + 16)) || (rc = c->in_off.ensure(((size_t)m + 1) * 8)) || (rc = c->norm_text.ensure((size_t)bytes + 16)) ||
            (rc = c->out_off.ensure(((size_t)cap + 1) * 8)) || (rc = c->span_out.ensure((size_t)cap * sizeof(kgpu_sentence) + 16))) return rc;
        if (bytes && (rc = ctx_h2d(c, c->in_utf8.p, utf8 + offsets[lo], (size_t)bytes, "H2D text"))) return rc;
        if ((rc = ctx_h2d(c, c->in_off.p, offsets + lo, ((size_t)m + 1) * 8, "H2D offsets"))) return rc;
        const uint8_t *d_in = (const uint8_t *)c->in_utf8.p - offsets[lo];   // (the offsets are as the caller has them)
        if ((rc = enqueue_sentences(c, d_in, (const uint64_t *)c->in_off.p, m, bytes, rule, (uint8_t *)c->norm_text.p, (uint64_t *)c->out_off.p,
                                    (kgpu_sentence *)c->span_out.p, cap, who))) return rc;
        uint64_t got = 0, kept = 0;
        rc = kgpu_ctx_sync_sentences(c, &got, &kept);
        if (rc != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
        if (rc == KGPU_ERR_CAPACITY) overflow = true;
        if (!overflow) {
            rel.resize((size_t)got + 1);
            if (hipMemcpy(rel.data(), c->out_off.p, ((size_t)got + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H offsets failed", who); return KGPU_ERR_HIP; }
            if (got && hipMemcpy(sents + S, c->span_out.p, (size_t)got * sizeof(kgpu_sentence), hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H records failed", who); return KGPU_ERR_HIP; }
            if (kept && hipMemcpy(out + at, c->norm_text.p, (size_t)kept, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H text failed", who); return KGPU_ERR_HIP; }
            for (uint64_t k = 0; k < got; ++k) { out_offsets[S + k] = at + rel[k]; sents[S + k].line += lo; }
            at += kept;
        }
        S += got;
        lo += m;
        if (!n) break;
    }
    *n_sentences = S;
    if (overflow) { set_error("%s: %llu sentences, capacity %llu", who, (unsigned long long)S, (unsigned long long)sent_capacity); return KGPU_ERR_CAPACITY; }
    out_offsets[S] = at;
    return KGPU_OK;
}
