// kanpyo_amd/csrc/kgpu_prob_batch.cpp -- kgpu_tokenize_batch_marginals, kgpu_tokenize_batch_samples: the lattice probabilities (include/kanpyo_gpu.h,
// "lattice probabilities") of n sentences in host memory.
//
// Two kept-lattice calls (kgpu_lattice_call.h has the protocol; DESIGN.md, "The kept-lattice protocol"): this file has their own part -- the launches of
// kgpu_prob.hip over a chunk's lattices, the probability slabs they keep behind them, and where the records go.  ONE ops type serves both: a call is
// marginals (n_samples == 0) or samples, and differs in which launches run and which arrays come back.
#include "kgpu_lattice_call.h"

namespace {

struct ProbOps : LatticeOps {
    const char *who;
    static constexpr LatticeHook hook = HOOK_PROB;
    static constexpr const char *measure_what = "probability launch";
    double theta; uint32_t select = 0; double min_prob = 0.0; uint32_t n_samples = 0; uint64_t seed = 0;
    kgpu_token *tokens; uint64_t token_capacity;
    double *probs = nullptr; uint8_t *on_best = nullptr; double *log_z = nullptr, *best_logprob = nullptr;   // marginals (tok_offsets: n + 1)
    uint64_t *path_offsets = nullptr; int32_t *costs = nullptr; uint64_t path_capacity = 0;                 // samples (tok_offsets: path_capacity + 1)
    uint64_t *tok_offsets;
    uint64_t *n_paths = nullptr, *n_tokens;
    ProbArgs g{};
    std::vector<uint64_t> poff, toff;

    bool samples() const { return n_samples != 0; }
    void begin() { if (path_offsets) path_offsets[0] = 0; tok_offsets[0] = 0; }
    // marginals  sent_len [m + 1] | log_z [m] | best_logprob [m];  samples  path_len [items + 1] | path_offsets [m + 1] | path_cost [items] (int32)
    size_t chunk_words(uint64_t m) const { const uint64_t items = m * n_samples; return samples() ? (size_t)(items + 1 + m + 1 + (items + 1) / 2 + 1) : (size_t)(3 * m + 2); }
    void fill(const LatticeChunk &f) {
        const uint64_t m = f.m, items = m * n_samples;
        g = ProbArgs{};
        g.n = m; g.sent_base = f.lo;   // (a sample's hash takes the sentence's index in the CALL: the chunks' cuts do not change what is drawn)
        g.theta = theta; g.min_prob = min_prob; g.select = select; g.n_samples = n_samples; g.seed = seed;
        g.ctl = f.ctl; g.arena = f.arena; g.arena_bytes = f.arena_bytes; g.desc = f.desc;
        g.conn = f.conn; g.conn_rows = f.conn_rows; g.status = f.status;
        uint64_t *w = f.words;
        if (samples()) { g.path_len = w; g.path_offsets = w + items + 1; g.path_cost = (int32_t *)(w + items + 1 + m + 1); }
        else { g.sent_len = w; g.log_z = (double *)(w + m + 1); g.best_logprob = g.log_z + m; }
    }
    int measure(hipStream_t st) { return samples() ? launch_prob_samples_measure(g, st) : launch_prob_marginals_measure(g, st); }
    void totals(const uint64_t *t[2]) const {   // the chunk's records; samples: and its paths
        if (samples()) { t[0] = g.path_len + g.n * n_samples; t[1] = g.path_offsets + g.n; }
        else t[0] = g.sent_len + g.n;
    }
    bool fits(const uint64_t done[2], const uint64_t sz[2]) const { return done[0] + sz[0] <= token_capacity && (!samples() || done[1] + sz[1] <= path_capacity); }
    // the output block: records [T] | marginals: probs [T] | on_best [T];  samples: tok_offsets [P + 1] | costs [P]
    size_t mid_bytes(const uint64_t sz[2]) const { return samples() ? (size_t)(sz[1] + 1) * 8 : (size_t)sz[0] * 8; }
    size_t out_bytes(const uint64_t sz[2]) const { return (size_t)sz[0] * sizeof(kgpu_token) + mid_bytes(sz) + (samples() ? (size_t)sz[1] * 4 : (size_t)sz[0]); }
    void place(uint8_t *blk, const uint64_t sz[2]) {
        const size_t o1 = (size_t)sz[0] * sizeof(kgpu_token), o2 = o1 + mid_bytes(sz);
        g.tokens = (kgpu_token *)blk; g.token_cap = sz[0];
        if (samples()) { g.tok_offsets = (uint64_t *)(blk + o1); g.costs = (int32_t *)(blk + o2); g.path_cap = sz[1]; }
        else { g.probs = (double *)(blk + o1); g.on_best = blk + o2; }
    }
    int write(hipStream_t st) { return samples() ? launch_prob_samples_write(g, st) : launch_prob_marginals_write(g, st); }
    // The records and the offsets are delivered only while nothing has overflowed (samples: tok_offsets is bounded by the path capacity).  Marginals: log_z and
    // best_logprob have n entries whatever the capacity is and are final behind the measure launches -- they are delivered regardless.
    hipError_t deliver(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits, const char *&what) {
        const uint64_t T = sz[0], P = sz[1], m = f.m;
        hipError_t e;
        if (fits) {
            what = "D2H records";
            if ((e = d2h(tokens + done[0], g.tokens, (size_t)T * sizeof(kgpu_token), f.stream)) != hipSuccess) return e;
            poff.resize((size_t)m + 1);
            if (samples()) {
                toff.resize((size_t)P + 1);
                what = "D2H costs";
                if ((e = d2h(costs + done[1], g.costs, (size_t)P * 4, f.stream)) != hipSuccess) return e;
                what = "D2H offsets";
                if ((e = d2h(toff.data(), g.tok_offsets, (size_t)(P + 1) * 8, f.stream)) != hipSuccess ||
                    (e = d2h(poff.data(), g.path_offsets, (size_t)(m + 1) * 8, f.stream)) != hipSuccess) return e;
            } else {
                what = "D2H marginals";
                if ((e = d2h(probs + done[0], g.probs, (size_t)T * 8, f.stream)) != hipSuccess || (e = d2h(on_best + done[0], g.on_best, (size_t)T, f.stream)) != hipSuccess) return e;
                what = "D2H offsets";
                if ((e = d2h(poff.data(), g.sent_len, (size_t)(m + 1) * 8, f.stream)) != hipSuccess) return e;
            }
        }
        if (samples()) return hipSuccess;
        what = "D2H log_z";
        if ((e = d2h(log_z + f.lo, g.log_z, (size_t)m * 8, f.stream)) != hipSuccess) return e;
        return d2h(best_logprob + f.lo, g.best_logprob, (size_t)m * 8, f.stream);
    }
    void fix_up(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits) {
        if (!fits) return;
        if (samples()) {
            for (uint64_t i = 0; i <= f.m; ++i) path_offsets[f.lo + i] = done[1] + poff[(size_t)i];
            for (uint64_t p = 0; p <= sz[1]; ++p) tok_offsets[done[1] + p] = done[0] + toff[(size_t)p];
        } else {
            for (uint64_t i = 0; i <= f.m; ++i) tok_offsets[f.lo + i] = done[0] + poff[(size_t)i];
        }
    }
    void report(const uint64_t done[2]) { if (n_paths) *n_paths = done[1]; *n_tokens = done[0]; }
    void too_small(const uint64_t done[2]) {
        if (samples())
            set_error("buffers too small: need %llu paths (capacity %llu) and %llu tokens (capacity %llu)", (unsigned long long)done[1], (unsigned long long)path_capacity,
                      (unsigned long long)done[0], (unsigned long long)token_capacity);
        else set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)done[0], (unsigned long long)token_capacity);
    }
};

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
    ProbOps k{};
    k.who = who; k.theta = theta; k.select = select; k.min_prob = min_prob;
    k.tokens = tokens; k.token_capacity = token_capacity; k.probs = probs; k.on_best = on_best; k.log_z = log_z; k.best_logprob = best_logprob;
    k.tok_offsets = tok_offsets; k.n_tokens = n_tokens;
    return lattice_call(k, d, utf8, offsets, n, status);
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
    ProbOps k{};
    k.who = who; k.theta = theta; k.n_samples = n_samples; k.seed = seed;
    k.tokens = tokens; k.token_capacity = token_capacity; k.path_offsets = path_offsets; k.costs = costs; k.path_capacity = path_capacity;
    k.tok_offsets = tok_offsets; k.n_paths = n_paths; k.n_tokens = n_tokens;
    return lattice_call(k, d, utf8, offsets, n, status);
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
