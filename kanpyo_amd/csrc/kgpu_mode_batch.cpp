// kanpyo_amd/csrc/kgpu_mode_batch.cpp -- kgpu_tokenize_batch_mode: the search / extended mode decode (include/kanpyo_gpu.h, "search mode") of n sentences
// in host memory.
//
// The protocol of kgpu_nbest_batch.cpp, in a file of its own (that file stays as it is): the call's chunks (cut by input bytes and sentences, so that the
// lattices and slabs a chunk keeps in the arena stay bounded; run one after the other on ONE pooled context: not a throughput path), a chunk's launches --
// the general kernel with BatchArgs::keep_lattice over the whole chunk, then the four launches of kgpu_mode.hip, one host wait between the scan and the
// write -- the arena_overflow protocol of the kept lattices and their slabs, and the delivery into the caller's buffers.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kgpu_mode_core.h"
#include "kgpu_runtime.h"

namespace {

constexpr uint64_t CHUNK_BYTES = 256u << 10, CHUNK_SENTS = 1024;   // a chunk's input: its lattices take a few hundred bytes per input byte, its slabs 8 bytes per node

struct Call {
    kgpu_dict *d; kgpu_ctx *c;
    const uint8_t *utf8; const uint64_t *offsets;
    kgpu_mode_opts opts;
    kgpu_token *tokens; uint64_t token_capacity;
    uint64_t *tok_offsets; int32_t *costs;
    uint8_t *status;
    uint64_t tokens_done = 0;
    bool overflow = false;
    std::vector<uint64_t> rel, toff;
    std::vector<uint8_t> st;
};

int hip_fail(Call &k, hipError_t e, const char *what) {
    set_error("kgpu_tokenize_batch_mode: %s: %s", what, hipGetErrorString(e));
    k.c->ctl_dirty = true;
    return KGPU_ERR_HIP;
}

// Sentences [lo, lo + m) of the call: lattices, forward, records, delivery behind what has been delivered.
int run_chunk(Call &k, uint64_t lo, uint64_t m) {
    kgpu_ctx *c = k.c;
    kgpu_dict *d = k.d;
    const uint64_t *off = k.offsets + lo;
    const uint64_t base = off[0], total = off[m] - base;
    int rc;
    // (the context's graphviz buffers serve: the descriptors, the scan's array with the costs behind it -- sent_len [m + 1] | costs [m] -- and the output block)
    if ((rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)token_bound(total, m) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure((size_t)m * 4 + 8)) || (rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure((size_t)(m + 1) * 8)) ||
        (rc = c->out_status.ensure((size_t)m + 16)) || (rc = c->gv_desc.ensure((size_t)m * LAT_DESC_WORDS * 8 + 8)) || (rc = c->gv_len.ensure((size_t)(m + 1) * 8 + (size_t)m * 4 + 8)))
        return rc;
    k.rel.resize((size_t)m + 1);
    for (uint64_t i = 0; i <= m; ++i) k.rel[(size_t)i] = off[i] - base;
    hipError_t e;
    // (every copy and launch goes on c->stream and is waited for below: no batch is begun -- as kgpu_lattice_dump)
    if (total && (e = hipMemcpyAsync(c->in_utf8.p, k.utf8 + base, (size_t)total, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    if ((e = hipMemcpyAsync(c->in_off.p, k.rel.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    ModeArgs g{};
    uint64_t T = 0;   // the chunk's records
    const TestHooks hooks = test_hooks();
    const size_t arena_max = hooks.mode_arena_max ? (size_t)hooks.mode_arena_max : ARENA_MAX;
    size_t limit = (size_t)hooks.mode_arena_initial;   // what of the arena the kept lattices and the slabs may use (0: all of it)
    for (;;) {
        BatchArgs a{};
        a.utf8 = (const uint8_t *)c->in_utf8.p; a.offsets = (const uint64_t *)c->in_off.p; a.n = m; a.ctl = c->d_ctl;
        a.arena = (uint8_t *)c->arena.p; a.arena_bytes = limit ? std::min(limit, c->arena.bytes) : c->arena.bytes;
        a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p; a.status = (uint8_t *)c->out_status.p;
        a.keep_lattice = 1; a.lat_desc = (unsigned long long *)c->gv_desc.p;
        g = ModeArgs{};
        g.n = m; g.opts = k.opts; g.ctl = a.ctl; g.arena = a.arena; g.arena_bytes = a.arena_bytes; g.utf8 = a.utf8; g.offsets = a.offsets; g.desc = a.lat_desc;
        g.conn = d->view.conn; g.conn_rows = d->view.conn_rows; g.status = a.status;
        g.sent_len = (uint64_t *)c->gv_len.p; g.costs = (int32_t *)(g.sent_len + m + 1);
        c->ctl_dirty = true;   // no scan kernel behind this launch: the next batch zeroes the block itself
        Control hc{};
        if ((e = hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream)) != hipSuccess ||
            (e = hipMemsetAsync(c->gv_desc.p, 0, (size_t)m * LAT_DESC_WORDS * 8 + 8, c->stream)) != hipSuccess) return hip_fail(k, e, "memset");
        if ((e = (hipError_t)launch_general_keep(d->view, a, c->stream)) != hipSuccess) return hip_fail(k, e, "lattice launch");
        if ((e = (hipError_t)launch_mode_measure(g, c->stream)) != hipSuccess) return hip_fail(k, e, "forward launch");
        if ((e = hipMemcpyAsync(&hc, c->d_ctl, sizeof(Control), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(&T, g.sent_len + m, 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
        if (!hc.arena_overflow) break;
        // the kept lattices and their slabs did not fit (the arena_overflow protocol): a bigger arena and the chunk once more; at the largest arena the chunk in
        // halves, and a sentence that alone does not fit keeps KGPU_SENT_NO_SCRATCH and has no records
        const size_t want = (limit ? std::min(limit, c->arena.bytes) : c->arena.bytes) * 2;
        if (want <= arena_max) { if ((rc = c->arena.ensure(want))) return rc; if (limit) limit = want; c->rt.arena_regrows++; continue; }
        if (m > 1) { if ((rc = run_chunk(k, lo, m / 2))) return rc; return run_chunk(k, lo + m / 2, m - m / 2); }
        break;
    }
    if (k.tokens_done + T > k.token_capacity) k.overflow = true;
    if (!k.overflow) {
        if ((rc = c->gv_text.ensure((size_t)T * sizeof(kgpu_token) + 16))) return rc;
        g.tokens = (kgpu_token *)c->gv_text.p; g.token_cap = T;
        if ((e = (hipError_t)launch_mode_write(g, c->stream)) != hipSuccess) return hip_fail(k, e, "write launch");
        if (T && (e = hipMemcpyAsync(k.tokens + k.tokens_done, g.tokens, (size_t)T * sizeof(kgpu_token), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H records");
    }
    k.toff.resize((size_t)m + 1);
    k.st.resize((size_t)m + 1);
    if ((e = hipMemcpyAsync(k.toff.data(), g.sent_len, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H offsets");
    if (k.costs && m && (e = hipMemcpyAsync(k.costs + lo, g.costs, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H costs");
    if (k.status && m && (e = hipMemcpyAsync(k.st.data(), c->out_status.p, (size_t)m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H status");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
    for (uint64_t i = 0; i <= m; ++i) k.tok_offsets[lo + i] = k.tokens_done + k.toff[(size_t)i];   // (the exact offsets, whether the records fit or not)
    if (k.status && m) std::memcpy(k.status + lo, k.st.data(), (size_t)m);
    k.tokens_done += T;
    return KGPU_OK;
}

}  // namespace

extern "C" int kgpu_tokenize_batch_mode(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_mode_opts *opts,
                                        kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs, uint8_t *status, uint64_t *n_tokens) {
    const char *who = "kgpu_tokenize_batch_mode";
    if (n_tokens) *n_tokens = 0;
    if (!d || !offsets || !opts || !tok_offsets || !n_tokens || (token_capacity && !tokens)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (!kgpu::mode_opts_valid(*opts)) { set_error("%s: mode %u is not 0, 1 or 2, or a reserved word is set", who, opts->mode); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = check_host_batch(who, offsets, n, utf8))) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] - offsets[i] >= (1ull << 31)) { set_error("%s: sentence %llu too long", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);
    if (lease.rc) return lease.rc;
    kgpu_ctx *c = lease.c;
    Call k{d, c, utf8, offsets, *opts, tokens, token_capacity, tok_offsets, costs, status};
    if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    rc = KGPU_OK;
    tok_offsets[0] = 0;
    const uint64_t hook = test_hooks().mode_chunk_sents, max_sents = hook ? hook : CHUNK_SENTS;
    for (uint64_t done = 0; !rc && done < n;) {
        uint64_t m = 0;
        while (done + m < n && m < max_sents && (m == 0 || offsets[done + m + 1] - offsets[done] <= CHUNK_BYTES)) ++m;
        rc = run_chunk(k, done, m);
        done += m;
    }
    *n_tokens = k.tokens_done;
    if (!rc && k.overflow) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)k.tokens_done, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return rc;
}
