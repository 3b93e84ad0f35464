// kanpyo_amd/csrc/kgpu_nbest_batch.cpp -- kgpu_tokenize_batch_nbest: the N-best paths (include/kanpyo_gpu.h, "N-best paths") of n sentences in host memory.
//
// A kept-lattice call (kgpu_lattice_call.h has the protocol; DESIGN.md, "The kept-lattice protocol"): this file has the call's own part -- the launches of
// kgpu_nbest.hip over a chunk's lattices, the lists they keep behind them, and where the paths go.
#include "kgpu_lattice_call.h"

namespace {

struct NbestOps : LatticeOps {
    const char *who = "kgpu_tokenize_batch_nbest";
    static constexpr LatticeHook hook = HOOK_NBEST;
    static constexpr const char *measure_what = "list launch";
    uint32_t k;
    kgpu_token *tokens; uint64_t token_capacity;
    uint64_t *path_offsets, *tok_offsets; int32_t *costs; uint64_t path_capacity;
    uint64_t *n_paths, *n_tokens;
    NbestArgs g{};
    std::vector<uint64_t> poff, toff;

    void begin() { path_offsets[0] = 0; tok_offsets[0] = 0; }
    // the scans' arrays: path_len [m k + 1] | path_offsets [m + 1]
    size_t chunk_words(uint64_t m) const { return (size_t)(m * k + m + 2); }
    void fill(const LatticeChunk &f) {
        g = NbestArgs{};
        g.n = f.m; g.k = k; g.ctl = f.ctl; g.arena = f.arena; g.arena_bytes = f.arena_bytes; g.desc = f.desc;
        g.conn = f.conn; g.conn_rows = f.conn_rows; g.status = f.status;
        g.path_len = f.words; g.path_offsets = g.path_len + f.m * k + 1;
    }
    int measure(hipStream_t st) { return launch_nbest_measure(g, st); }
    void totals(const uint64_t *t[2]) const { t[0] = g.path_len + g.n * k; t[1] = g.path_offsets + g.n; }   // the chunk's records, its paths
    bool fits(const uint64_t done[2], const uint64_t sz[2]) const { return done[0] + sz[0] <= token_capacity && done[1] + sz[1] <= path_capacity; }
    // the output block: records [T] | tok_offsets [P + 1] | costs [P]
    size_t out_bytes(const uint64_t sz[2]) const { return (size_t)sz[0] * sizeof(kgpu_token) + (size_t)(sz[1] + 1) * 8 + (size_t)sz[1] * 4; }
    void place(uint8_t *blk, const uint64_t sz[2]) {
        const size_t o_toff = (size_t)sz[0] * sizeof(kgpu_token), o_cost = o_toff + (size_t)(sz[1] + 1) * 8;
        g.tokens = (kgpu_token *)blk; g.token_cap = sz[0]; g.tok_offsets = (uint64_t *)(blk + o_toff); g.costs = (int32_t *)(blk + o_cost); g.path_cap = sz[1];
    }
    int write(hipStream_t st) { return launch_nbest_write(g, st); }
    // Everything, the offsets included, is delivered only while nothing has overflowed: tok_offsets has path_capacity + 1 entries, so the offsets of paths
    // that did not fit have nowhere to go.
    hipError_t deliver(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits, const char *&what) {
        if (!fits) return hipSuccess;
        const uint64_t T = sz[0], P = sz[1];
        hipError_t e;
        poff.resize((size_t)f.m + 1); toff.resize((size_t)P + 1);
        what = "D2H records";
        if ((e = d2h(tokens + done[0], g.tokens, (size_t)T * sizeof(kgpu_token), f.stream)) != hipSuccess) return e;
        what = "D2H costs";
        if ((e = d2h(costs + done[1], g.costs, (size_t)P * 4, f.stream)) != hipSuccess) return e;
        what = "D2H offsets";
        if ((e = d2h(toff.data(), g.tok_offsets, (size_t)(P + 1) * 8, f.stream)) != hipSuccess) return e;
        return d2h(poff.data(), g.path_offsets, (size_t)(f.m + 1) * 8, f.stream);
    }
    void fix_up(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits) {
        if (!fits) return;
        for (uint64_t i = 0; i <= f.m; ++i) path_offsets[f.lo + i] = done[1] + poff[(size_t)i];
        for (uint64_t p = 0; p <= sz[1]; ++p) tok_offsets[done[1] + p] = done[0] + toff[(size_t)p];
    }
    void report(const uint64_t done[2]) { *n_paths = done[1]; *n_tokens = done[0]; }
    void too_small(const uint64_t done[2]) {
        set_error("buffers too small: need %llu paths (capacity %llu) and %llu tokens (capacity %llu)", (unsigned long long)done[1], (unsigned long long)path_capacity,
                  (unsigned long long)done[0], (unsigned long long)token_capacity);
    }
};

}  // namespace

extern "C" int kgpu_tokenize_batch_nbest(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint32_t n_best,
                                         kgpu_token *tokens, uint64_t token_capacity, uint64_t *path_offsets, uint64_t *tok_offsets, int32_t *costs,
                                         uint64_t path_capacity, uint8_t *status, uint64_t *n_paths, uint64_t *n_tokens) {
    NbestOps ops;
    const char *who = ops.who;
    if (n_paths) *n_paths = 0;
    if (n_tokens) *n_tokens = 0;
    if (!d || !offsets || !path_offsets || !tok_offsets || !n_paths || !n_tokens || (token_capacity && !tokens) || (path_capacity && !costs)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (n_best < 1 || n_best > KGPU_NBEST_MAX) { set_error("%s: n_best %u is outside 1 .. %d", who, n_best, KGPU_NBEST_MAX); return KGPU_ERR_INVALID_ARG; }
    ops.k = n_best; ops.tokens = tokens; ops.token_capacity = token_capacity; ops.path_offsets = path_offsets; ops.tok_offsets = tok_offsets; ops.costs = costs;
    ops.path_capacity = path_capacity; ops.n_paths = n_paths; ops.n_tokens = n_tokens;
    return lattice_call(ops, d, utf8, offsets, n, status);
}
