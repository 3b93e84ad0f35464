// kanpyo_amd/csrc/kgpu_graphviz_host.cpp -- kgpu_graphviz_batch: the reference's `kanpyo graphviz` (src/bin/kanpyo.rs:127-148 over
// src/graphviz.rs:30-163) for n sentences in host memory.
//
// Owns: the call's chunks (cut by input bytes and sentences, so that the lattices a chunk keeps in the arena stay bounded; run one after the
// other on ONE pooled context: not a throughput path), a chunk's launches -- the general kernel with BatchArgs::keep_lattice over the whole
// chunk, then the four render launches of kgpu_graphviz.hip: five launches whatever the chunk holds, one host wait between the lengths and the
// write -- the arena_overflow protocol of the kept lattices, and the delivery into the caller's buffers (the kgpu_tokenize_batch_lines protocol).
#include <algorithm>
#include <cstring>
#include <vector>

#include "kgpu_runtime.h"

namespace {

constexpr uint64_t CHUNK_BYTES = 256u << 10, CHUNK_SENTS = 1024;   // a chunk's input: its lattices take a few hundred bytes per input byte

struct Call {
    kgpu_dict *d; kgpu_ctx *c;
    const uint8_t *utf8; const uint64_t *offsets;
    uint64_t dpi; int full_state;
    uint8_t *text; uint64_t text_capacity; uint64_t *text_offsets; uint8_t *status;
    uint64_t text_done = 0;
    bool overflow = false;
    std::vector<uint64_t> rel, toff;
    std::vector<uint8_t> st;
};

int hip_fail(Call &k, hipError_t e, const char *what) {
    set_error("kgpu_graphviz_batch: %s: %s", what, hipGetErrorString(e));
    k.c->ctl_dirty = true;
    return KGPU_ERR_HIP;
}

// Sentences [lo, lo + m) of the call: lattices, documents, delivery behind what has been delivered.
int run_chunk(Call &k, uint64_t lo, uint64_t m) {
    kgpu_ctx *c = k.c;
    kgpu_dict *d = k.d;
    const uint64_t *off = k.offsets + lo;
    const uint64_t base = off[0], total = off[m] - base;
    int rc;
    if ((rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)token_bound(total, m) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure((size_t)m * 4 + 8)) || (rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure((size_t)(m + 1) * 8)) ||
        (rc = c->out_status.ensure((size_t)m + 16)) || (rc = c->gv_desc.ensure((size_t)m * LAT_DESC_WORDS * 8 + 8)) || (rc = c->gv_len.ensure((size_t)(m + 1) * 8)))
        return rc;
    k.rel.resize((size_t)m + 1);
    for (uint64_t i = 0; i <= m; ++i) k.rel[(size_t)i] = off[i] - base;
    hipError_t e;
    // (every copy and launch goes on c->stream and is waited for below: no batch is begun -- as kgpu_lattice_dump)
    if (total && (e = hipMemcpyAsync(c->in_utf8.p, k.utf8 + base, (size_t)total, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    if ((e = hipMemcpyAsync(c->in_off.p, k.rel.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    GraphvizArgs g{};
    uint64_t bytes = 0;
    const TestHooks hooks = test_hooks();
    const size_t arena_max = hooks.graphviz_arena_max ? (size_t)hooks.graphviz_arena_max : ARENA_MAX;
    size_t limit = (size_t)hooks.graphviz_arena_initial;   // what of the arena the kept lattices may use (0: all of it)
    for (;;) {
        BatchArgs a{};
        a.utf8 = (const uint8_t *)c->in_utf8.p; a.offsets = (const uint64_t *)c->in_off.p; a.n = m; a.ctl = c->d_ctl;
        a.arena = (uint8_t *)c->arena.p; a.arena_bytes = limit ? std::min(limit, c->arena.bytes) : c->arena.bytes;
        a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p; a.status = (uint8_t *)c->out_status.p;
        a.keep_lattice = 1; a.lat_desc = (unsigned long long *)c->gv_desc.p;
        g = GraphvizArgs{};
        g.utf8 = a.utf8; g.offsets = a.offsets; g.n = m; g.arena = a.arena; g.desc = a.lat_desc;
        g.conn = d->view.conn; g.conn_rows = d->view.conn_rows;
        g.label = d->label; g.label_off = d->label_off; g.n_morph = (uint32_t)d->info.n_morphs;
        g.full_state = k.full_state ? 1u : 0u; g.dpi = k.dpi;
        g.sent_len = (uint64_t *)c->gv_len.p;
        c->ctl_dirty = true;   // no scan kernel behind this launch: the next batch zeroes the block itself
        Control hc{};
        if ((e = hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream)) != hipSuccess ||
            (e = hipMemsetAsync(c->gv_desc.p, 0, (size_t)m * LAT_DESC_WORDS * 8 + 8, c->stream)) != hipSuccess) return hip_fail(k, e, "memset");
        if ((e = (hipError_t)launch_general_keep(d->view, a, c->stream)) != hipSuccess) return hip_fail(k, e, "lattice launch");
        if ((e = (hipError_t)launch_graphviz_measure(g, c->stream)) != hipSuccess) return hip_fail(k, e, "render launch");
        if ((e = hipMemcpyAsync(&hc, c->d_ctl, sizeof(Control), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(&bytes, g.sent_len + m, 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
        if (!hc.arena_overflow) break;
        // the kept lattices did not fit (the arena_overflow protocol): a bigger arena and the chunk once more; at the largest arena the chunk in halves, and a
        // sentence that alone does not fit keeps KGPU_SENT_NO_SCRATCH and renders to nothing
        const size_t want = (limit ? std::min(limit, c->arena.bytes) : c->arena.bytes) * 2;
        if (want <= arena_max) { if ((rc = c->arena.ensure(want))) return rc; if (limit) limit = want; c->rt.arena_regrows++; continue; }
        if (m > 1) { if ((rc = run_chunk(k, lo, m / 2))) return rc; return run_chunk(k, lo + m / 2, m - m / 2); }
        break;
    }
    if (k.text_done + bytes > k.text_capacity) k.overflow = true;
    if (!k.overflow) {
        if ((rc = c->gv_text.ensure((size_t)bytes + 16))) return rc;
        g.text = (uint8_t *)c->gv_text.p; g.text_cap = bytes;
        if ((e = (hipError_t)launch_graphviz_write(g, c->stream)) != hipSuccess) return hip_fail(k, e, "write launch");
        k.toff.resize((size_t)m + 1);
        if (bytes && (e = hipMemcpyAsync(k.text + k.text_done, g.text, (size_t)bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H text");
        if ((e = hipMemcpyAsync(k.toff.data(), g.sent_len, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H offsets");
    }
    k.st.resize((size_t)m + 1);
    if (k.status && m && (e = hipMemcpyAsync(k.st.data(), c->out_status.p, (size_t)m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H status");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
    if (!k.overflow) for (uint64_t i = 0; i <= m; ++i) k.text_offsets[lo + i] = k.text_done + k.toff[(size_t)i];
    if (k.status && m) std::memcpy(k.status + lo, k.st.data(), (size_t)m);
    k.text_done += bytes;
    return KGPU_OK;
}

}  // namespace

extern "C" int kgpu_graphviz_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint64_t dpi, int full_state,
                                   uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    const char *who = "kgpu_graphviz_batch";
    if (!d || !offsets || !text_offsets || (text_capacity && !text)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = check_host_batch(who, offsets, n, utf8)) || (rc = require_features(d, who))) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] - offsets[i] >= (1ull << 31)) { set_error("%s: sentence %llu too long", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    if ((rc = ensure_label_pool(d))) return rc;
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    if (lease.rc) return lease.rc;
    kgpu_ctx *c = lease.c;
    Call k{d, c, utf8, offsets, dpi, full_state, text, text_capacity, text_offsets, status};
    if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    rc = KGPU_OK;
    text_offsets[0] = 0;
    const uint64_t hook = test_hooks().graphviz_chunk_sents, max_sents = hook ? hook : CHUNK_SENTS;
    for (uint64_t done = 0; !rc && done < n;) {
        uint64_t m = 0;
        while (done + m < n && m < max_sents && (m == 0 || offsets[done + m + 1] - offsets[done] <= CHUNK_BYTES)) ++m;
        rc = run_chunk(k, done, m);
        done += m;
    }
    if (n_bytes) *n_bytes = k.text_done;
    if (!rc && k.overflow) {
        set_error("text buffer too small: need %llu, capacity %llu", (unsigned long long)k.text_done, (unsigned long long)text_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return rc;
}
