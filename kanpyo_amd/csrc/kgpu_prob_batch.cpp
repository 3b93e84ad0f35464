// kanpyo_amd/csrc/kgpu_prob_batch.cpp -- kgpu_tokenize_batch_marginals, kgpu_tokenize_batch_samples: the lattice probabilities (include/kanpyo_gpu.h,
// "lattice probabilities") of n sentences in host memory.
//
// The protocol of kgpu_nbest_batch.cpp, in a file of its own (that file stays as it is): the call's chunks (cut by input bytes and sentences, so that the
// lattices and slabs a chunk keeps in the arena stay bounded; run one after the other on ONE pooled context: not a throughput path), a chunk's launches --
// the general kernel with BatchArgs::keep_lattice over the whole chunk, then the launches of kgpu_prob.hip, one host wait between the scan and the write --
// the arena_overflow protocol of the kept lattices and their slabs, and the delivery into the caller's buffers.  ONE chunk loop serves both calls: a call
// is marginals (n_samples == 0) or samples, and differs in which launches run and which arrays come back.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kgpu_runtime.h"

namespace {

constexpr uint64_t CHUNK_BYTES = 256u << 10, CHUNK_SENTS = 1024;   // a chunk's input: its lattices take a few hundred bytes per input byte, its slabs 8 to 17 per node

struct Call {
    const char *who;
    kgpu_dict *d; kgpu_ctx *c;
    const uint8_t *utf8; const uint64_t *offsets;
    double theta; uint32_t select; double min_prob; uint32_t n_samples; uint64_t seed;
    kgpu_token *tokens; uint64_t token_capacity;
    double *probs; uint8_t *on_best; double *log_z, *best_logprob;                 // marginals (tok_offsets: n + 1)
    uint64_t *path_offsets; int32_t *costs; uint64_t path_capacity;               // samples (tok_offsets: path_capacity + 1)
    uint64_t *tok_offsets;
    uint8_t *status;
    uint64_t paths_done = 0, tokens_done = 0;
    bool overflow = false;
    std::vector<uint64_t> rel, poff, toff;
    std::vector<uint8_t> st;
};

int hip_fail(Call &k, hipError_t e, const char *what) {
    set_error("%s: %s: %s", k.who, what, hipGetErrorString(e));
    k.c->ctl_dirty = true;
    return KGPU_ERR_HIP;
}

// Sentences [lo, lo + m) of the call: lattices, slabs, records, delivery behind what has been delivered.
int run_chunk(Call &k, uint64_t lo, uint64_t m) {
    kgpu_ctx *c = k.c;
    kgpu_dict *d = k.d;
    const bool samples = k.n_samples != 0;
    const uint64_t *off = k.offsets + lo;
    const uint64_t base = off[0], total = off[m] - base, items = m * k.n_samples;
    int rc;
    // (the context's graphviz buffers serve, as they serve N-best: the descriptors, the per-sentence arrays, the output block)
    // gv_len, 8-byte words: marginals  sent_len [m + 1] | log_z [m] | best_logprob [m];  samples  path_len [items + 1] | path_offsets [m + 1] | path_cost [items] (int32)
    const size_t len_words = samples ? (size_t)(items + 1 + m + 1 + (items + 1) / 2 + 1) : (size_t)(3 * m + 2);
    if ((rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)token_bound(total, m) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure((size_t)m * 4 + 8)) || (rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure((size_t)(m + 1) * 8)) ||
        (rc = c->out_status.ensure((size_t)m + 16)) || (rc = c->gv_desc.ensure((size_t)m * LAT_DESC_WORDS * 8 + 8)) || (rc = c->gv_len.ensure(len_words * 8)))
        return rc;
    k.rel.resize((size_t)m + 1);
    for (uint64_t i = 0; i <= m; ++i) k.rel[(size_t)i] = off[i] - base;
    hipError_t e;
    // (every copy and launch goes on c->stream and is waited for below: no batch is begun -- as kgpu_lattice_dump)
    if (total && (e = hipMemcpyAsync(c->in_utf8.p, k.utf8 + base, (size_t)total, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    if ((e = hipMemcpyAsync(c->in_off.p, k.rel.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(k, e, "H2D");
    ProbArgs g{};
    uint64_t sizes[2] = {0, 0};   // the chunk's records, its paths
    const TestHooks hooks = test_hooks();
    const size_t arena_max = hooks.prob_arena_max ? (size_t)hooks.prob_arena_max : ARENA_MAX;
    size_t limit = (size_t)hooks.prob_arena_initial;   // what of the arena the kept lattices and the slabs may use (0: all of it)
    for (;;) {
        BatchArgs a{};
        a.utf8 = (const uint8_t *)c->in_utf8.p; a.offsets = (const uint64_t *)c->in_off.p; a.n = m; a.ctl = c->d_ctl;
        a.arena = (uint8_t *)c->arena.p; a.arena_bytes = limit ? std::min(limit, c->arena.bytes) : c->arena.bytes;
        a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p; a.status = (uint8_t *)c->out_status.p;
        a.keep_lattice = 1; a.lat_desc = (unsigned long long *)c->gv_desc.p;
        g = ProbArgs{};
        g.n = m; g.sent_base = lo; g.theta = k.theta; g.min_prob = k.min_prob; g.select = k.select; g.n_samples = k.n_samples; g.seed = k.seed;
        g.ctl = a.ctl; g.arena = a.arena; g.arena_bytes = a.arena_bytes; g.desc = a.lat_desc;
        g.conn = d->view.conn; g.conn_rows = d->view.conn_rows; g.status = a.status;
        uint64_t *w = (uint64_t *)c->gv_len.p;
        if (samples) { g.path_len = w; g.path_offsets = w + items + 1; g.path_cost = (int32_t *)(w + items + 1 + m + 1); }
        else { g.sent_len = w; g.log_z = (double *)(w + m + 1); g.best_logprob = g.log_z + m; }
        c->ctl_dirty = true;   // no scan kernel behind this launch: the next batch zeroes the block itself
        Control hc{};
        if ((e = hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream)) != hipSuccess ||
            (e = hipMemsetAsync(c->gv_desc.p, 0, (size_t)m * LAT_DESC_WORDS * 8 + 8, c->stream)) != hipSuccess) return hip_fail(k, e, "memset");
        if ((e = (hipError_t)launch_general_keep(d->view, a, c->stream)) != hipSuccess) return hip_fail(k, e, "lattice launch");
        if ((e = (hipError_t)(samples ? launch_prob_samples_measure(g, c->stream) : launch_prob_marginals_measure(g, c->stream))) != hipSuccess) return hip_fail(k, e, "probability launch");
        if ((e = hipMemcpyAsync(&hc, c->d_ctl, sizeof(Control), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(&sizes[0], samples ? g.path_len + items : g.sent_len + m, 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (samples && (e = hipMemcpyAsync(&sizes[1], g.path_offsets + m, 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)) return hip_fail(k, e, "D2H");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
        if (!hc.arena_overflow) break;
        // the kept lattices and their slabs did not fit (the arena_overflow protocol): a bigger arena and the chunk once more; at the largest arena the chunk in
        // halves, and a sentence that alone does not fit keeps KGPU_SENT_NO_SCRATCH and has no records
        const size_t want = (limit ? std::min(limit, c->arena.bytes) : c->arena.bytes) * 2;
        if (want <= arena_max) { if ((rc = c->arena.ensure(want))) return rc; if (limit) limit = want; c->rt.arena_regrows++; continue; }
        if (m > 1) { if ((rc = run_chunk(k, lo, m / 2))) return rc; return run_chunk(k, lo + m / 2, m - m / 2); }
        break;
    }
    const uint64_t T = sizes[0], P = sizes[1];
    if (k.tokens_done + T > k.token_capacity || (samples && k.paths_done + P > k.path_capacity)) k.overflow = true;
    if (!k.overflow) {
        // the output block: records [T] | marginals: probs [T] | on_best [T];  samples: tok_offsets [P + 1] | costs [P]
        const size_t o1 = (size_t)T * sizeof(kgpu_token), o2 = o1 + (samples ? (size_t)(P + 1) * 8 : (size_t)T * 8);
        if ((rc = c->gv_text.ensure(o2 + (samples ? (size_t)P * 4 : (size_t)T) + 16))) return rc;
        uint8_t *blk = (uint8_t *)c->gv_text.p;
        g.tokens = (kgpu_token *)blk; g.token_cap = T;
        if (samples) { g.tok_offsets = (uint64_t *)(blk + o1); g.costs = (int32_t *)(blk + o2); g.path_cap = P; }
        else { g.probs = (double *)(blk + o1); g.on_best = blk + o2; }
        if ((e = (hipError_t)(samples ? launch_prob_samples_write(g, c->stream) : launch_prob_marginals_write(g, c->stream))) != hipSuccess) return hip_fail(k, e, "write launch");
        if (T && (e = hipMemcpyAsync(k.tokens + k.tokens_done, g.tokens, (size_t)T * sizeof(kgpu_token), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H records");
        k.poff.resize((size_t)m + 1);
        if (samples) {
            k.toff.resize((size_t)P + 1);
            if (P && (e = hipMemcpyAsync(k.costs + k.paths_done, g.costs, (size_t)P * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H costs");
            if ((e = hipMemcpyAsync(k.toff.data(), g.tok_offsets, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                (e = hipMemcpyAsync(k.poff.data(), g.path_offsets, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H offsets");
        } else {
            if (T && ((e = hipMemcpyAsync(k.probs + k.tokens_done, g.probs, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                      (e = hipMemcpyAsync(k.on_best + k.tokens_done, g.on_best, (size_t)T, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)) return hip_fail(k, e, "D2H marginals");
            if ((e = hipMemcpyAsync(k.poff.data(), g.sent_len, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H offsets");
        }
    }
    if (!samples && m && ((e = hipMemcpyAsync(k.log_z + lo, g.log_z, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                          (e = hipMemcpyAsync(k.best_logprob + lo, g.best_logprob, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)) return hip_fail(k, e, "D2H log_z");
    k.st.resize((size_t)m + 1);
    if (k.status && m && (e = hipMemcpyAsync(k.st.data(), c->out_status.p, (size_t)m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return hip_fail(k, e, "D2H status");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(k, e, "sync");
    if (!k.overflow) {
        if (samples) {
            for (uint64_t i = 0; i <= m; ++i) k.path_offsets[lo + i] = k.paths_done + k.poff[(size_t)i];
            for (uint64_t p = 0; p <= P; ++p) k.tok_offsets[k.paths_done + p] = k.tokens_done + k.toff[(size_t)p];
        } else {
            for (uint64_t i = 0; i <= m; ++i) k.tok_offsets[lo + i] = k.tokens_done + k.poff[(size_t)i];
        }
    }
    if (k.status && m) std::memcpy(k.status + lo, k.st.data(), (size_t)m);
    k.tokens_done += T; k.paths_done += P;
    return KGPU_OK;
}

// The chunk loop of both calls, behind their argument checks.
int run_call(Call &k, uint64_t n) {
    int rc;
    if ((rc = check_host_batch(k.who, k.offsets, n, k.utf8))) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (k.offsets[i + 1] - k.offsets[i] >= (1ull << 31)) { set_error("%s: sentence %llu too long", k.who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(k.d->device));
    PooledCtx lease(k.d);
    if (lease.rc) return lease.rc;
    kgpu_ctx *c = k.c = lease.c;
    if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    rc = KGPU_OK;
    if (k.path_offsets) k.path_offsets[0] = 0;
    k.tok_offsets[0] = 0;
    const uint64_t hook = test_hooks().prob_chunk_sents, max_sents = hook ? hook : CHUNK_SENTS;
    for (uint64_t done = 0; !rc && done < n;) {
        uint64_t m = 0;
        while (done + m < n && m < max_sents && (m == 0 || k.offsets[done + m + 1] - k.offsets[done] <= CHUNK_BYTES)) ++m;
        rc = run_chunk(k, done, m);
        done += m;
    }
    return rc;
}

bool theta_ok(double theta) { return theta > 0.0 && theta <= KGPU_THETA_MAX; }   // (false for a NaN)

}  // namespace

extern "C" int kgpu_tokenize_batch_marginals(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, double theta, uint32_t select, double min_prob,
                                             kgpu_token *tokens, uint64_t token_capacity, double *probs, uint8_t *on_best, uint64_t *tok_offsets, double *log_z,
                                             double *best_logprob, uint8_t *status, uint64_t *n_tokens) {
    const char *who = "kgpu_tokenize_batch_marginals";
    if (n_tokens) *n_tokens = 0;
    if (!d || !offsets || !tok_offsets || !n_tokens || (n && (!log_z || !best_logprob)) || (token_capacity && (!tokens || !probs || !on_best))) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (!theta_ok(theta)) { set_error("%s: theta is not a double above 0 and at most 2^64", who); return KGPU_ERR_INVALID_ARG; }
    if (select != KGPU_MARGINAL_BEST && select != KGPU_MARGINAL_ALL) { set_error("%s: select is neither KGPU_MARGINAL_BEST nor KGPU_MARGINAL_ALL", who); return KGPU_ERR_INVALID_ARG; }
    if (!(min_prob >= 0.0 && min_prob <= 1.0)) { set_error("%s: min_prob is outside [0, 1]", who); return KGPU_ERR_INVALID_ARG; }
    Call k{};
    k.who = who; k.d = d; k.utf8 = utf8; k.offsets = offsets; k.theta = theta; k.select = select; k.min_prob = min_prob;
    k.tokens = tokens; k.token_capacity = token_capacity; k.probs = probs; k.on_best = on_best; k.log_z = log_z; k.best_logprob = best_logprob;
    k.tok_offsets = tok_offsets; k.status = status;
    const int rc = run_call(k, n);
    *n_tokens = k.tokens_done;
    if (!rc && k.overflow) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)k.tokens_done, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return rc;
}

extern "C" int kgpu_tokenize_batch_samples(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, double theta, uint32_t n_samples, uint64_t seed,
                                           kgpu_token *tokens, uint64_t token_capacity, uint64_t *path_offsets, uint64_t *tok_offsets, int32_t *costs,
                                           uint64_t path_capacity, uint8_t *status, uint64_t *n_paths, uint64_t *n_tokens) {
    const char *who = "kgpu_tokenize_batch_samples";
    if (n_paths) *n_paths = 0;
    if (n_tokens) *n_tokens = 0;
    if (!d || !offsets || !path_offsets || !tok_offsets || !n_paths || !n_tokens || (token_capacity && !tokens) || (path_capacity && !costs)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (!theta_ok(theta)) { set_error("%s: theta is not a double above 0 and at most 2^64", who); return KGPU_ERR_INVALID_ARG; }
    if (n_samples < 1 || n_samples > KGPU_SAMPLES_MAX) { set_error("%s: n_samples %u is outside 1 .. %d", who, n_samples, KGPU_SAMPLES_MAX); return KGPU_ERR_INVALID_ARG; }
    Call k{};
    k.who = who; k.d = d; k.utf8 = utf8; k.offsets = offsets; k.theta = theta; k.n_samples = n_samples; k.seed = seed;
    k.tokens = tokens; k.token_capacity = token_capacity; k.path_offsets = path_offsets; k.costs = costs; k.path_capacity = path_capacity;
    k.tok_offsets = tok_offsets; k.status = status;
    const int rc = run_call(k, n);
    *n_paths = k.paths_done; *n_tokens = k.tokens_done;
    if (!rc && k.overflow) {
        set_error("buffers too small: need %llu paths (capacity %llu) and %llu tokens (capacity %llu)", (unsigned long long)k.paths_done, (unsigned long long)path_capacity,
                  (unsigned long long)k.tokens_done, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return rc;
}

// (tests) kexp (which = 0) / klog (which = 1) over n doubles on a device: what the device's arithmetic gives for the two functions alone
extern "C" int kgpu_debug_prob_device(int device, uint32_t which, const double *x, uint64_t n, double *out) {
    if (!x || !out || which > 1) { set_error("kgpu_debug_prob_device: bad argument"); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(device));
    double *dx = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void **)&dx, (size_t)n * 8 + 8);
    if (e == hipSuccess) e = hipMalloc((void **)&dout, (size_t)n * 8 + 8);
    if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = (hipError_t)launch_prob_eval(dx, n, dout, which, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dx); (void)hipFree(dout);
    if (e != hipSuccess) { set_error("kgpu_debug_prob_device: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    return KGPU_OK;
}
