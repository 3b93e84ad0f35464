// kanpyo_amd/csrc/kgpu_mode_batch.cpp -- kgpu_tokenize_batch_mode: the search / extended mode decode (include/kanpyo_gpu.h, "search mode") of n sentences
// in host memory.
//
// A kept-lattice call (kgpu_lattice_call.h has the protocol; DESIGN.md, "The kept-lattice protocol"): this file has the call's own part -- the launches of
// kgpu_mode.hip over a chunk's lattices, the state and kanji counts they keep behind them, and where the records and costs go.
#include "kgpu_lattice_call.h"
#include "kgpu_mode_core.h"

namespace {

struct ModeOps : LatticeOps {
    const char *who = "kgpu_tokenize_batch_mode";
    static constexpr LatticeHook hook = HOOK_MODE;
    static constexpr const char *measure_what = "forward launch";
    kgpu_mode_opts opts;
    kgpu_token *tokens; uint64_t token_capacity;
    uint64_t *tok_offsets; int32_t *costs;
    uint64_t *n_tokens;
    ModeArgs g{};
    std::vector<uint64_t> toff;

    void begin() { tok_offsets[0] = 0; }
    // the scan's array with the costs behind it: sent_len [m + 1] | costs [m] (int32)
    size_t chunk_words(uint64_t m) const { return (size_t)(m + 1 + (m + 1) / 2 + 1); }
    void fill(const LatticeChunk &f) {
        g = ModeArgs{};
        g.n = f.m; g.opts = opts; g.ctl = f.ctl; g.arena = f.arena; g.arena_bytes = f.arena_bytes; g.utf8 = f.utf8; g.offsets = f.offsets; g.desc = f.desc;
        g.conn = f.conn; g.conn_rows = f.conn_rows; g.status = f.status;
        g.sent_len = f.words; g.costs = (int32_t *)(g.sent_len + f.m + 1);
    }
    int measure(hipStream_t st) { return launch_mode_measure(g, st); }
    void totals(const uint64_t *t[2]) const { t[0] = g.sent_len + g.n; }   // the chunk's records
    bool fits(const uint64_t done[2], const uint64_t sz[2]) const { return done[0] + sz[0] <= token_capacity; }
    size_t out_bytes(const uint64_t sz[2]) const { return (size_t)sz[0] * sizeof(kgpu_token); }
    void place(uint8_t *blk, const uint64_t sz[2]) { g.tokens = (kgpu_token *)blk; g.token_cap = sz[0]; }
    int write(hipStream_t st) { return launch_mode_write(g, st); }
    // tok_offsets and costs have n entries whatever the capacity is, and the measure launches made them: they are delivered whether or not the records
    // fit -- the caller of a call that returned KGPU_ERR_CAPACITY has the exact offsets.
    hipError_t deliver(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits, const char *&what) {
        hipError_t e;
        what = "D2H records";
        if (fits && (e = d2h(tokens + done[0], g.tokens, (size_t)sz[0] * sizeof(kgpu_token), f.stream)) != hipSuccess) return e;
        toff.resize((size_t)f.m + 1);
        what = "D2H offsets";
        if ((e = d2h(toff.data(), g.sent_len, (size_t)(f.m + 1) * 8, f.stream)) != hipSuccess) return e;
        what = "D2H costs";
        return costs ? d2h(costs + f.lo, g.costs, (size_t)f.m * 4, f.stream) : hipSuccess;
    }
    void fix_up(const LatticeChunk &f, const uint64_t done[2], const uint64_t *, bool) {
        for (uint64_t i = 0; i <= f.m; ++i) tok_offsets[f.lo + i] = done[0] + toff[(size_t)i];
    }
    void report(const uint64_t done[2]) { *n_tokens = done[0]; }
    void too_small(const uint64_t done[2]) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)done[0], (unsigned long long)token_capacity);
    }
};

}  // namespace

extern "C" int kgpu_tokenize_batch_mode(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_mode_opts *opts,
                                        kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs, uint8_t *status, uint64_t *n_tokens) {
    ModeOps ops;
    const char *who = ops.who;
    if (n_tokens) *n_tokens = 0;
    if (!d || !offsets || !opts || !tok_offsets || !n_tokens || (token_capacity && !tokens)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (!kgpu::mode_opts_valid(*opts)) { set_error("%s: mode %u is not 0, 1 or 2, or a reserved word is set", who, opts->mode); return KGPU_ERR_INVALID_ARG; }
    ops.opts = *opts; ops.tokens = tokens; ops.token_capacity = token_capacity; ops.tok_offsets = tok_offsets; ops.costs = costs; ops.n_tokens = n_tokens;
    return lattice_call(ops, d, utf8, offsets, n, status);
}
