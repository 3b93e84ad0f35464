// kanpyo_amd/csrc/kgpu_graphviz_host.cpp -- kgpu_graphviz_batch: the reference's `kanpyo graphviz` (src/bin/kanpyo.rs:127-148 over
// src/graphviz.rs:30-163) for n sentences in host memory.
//
// A kept-lattice call (kgpu_lattice_call.h has the protocol; DESIGN.md, "The kept-lattice protocol"): this file has the call's own part -- the four render
// launches of kgpu_graphviz.hip over a chunk's lattices (five launches a chunk whatever it holds, one host wait between the lengths and the write), and
// where the documents go (the kgpu_tokenize_batch_lines protocol).
#include "kgpu_lattice_call.h"

namespace {

struct GraphvizOps : LatticeOps {
    const char *who = "kgpu_graphviz_batch";
    static constexpr LatticeHook hook = HOOK_GRAPHVIZ;
    static constexpr const char *measure_what = "render launch";
    kgpu_dict *d;
    uint64_t dpi; int full_state;
    uint8_t *text; uint64_t text_capacity; uint64_t *text_offsets;
    uint64_t *n_bytes;   // optional, alone among the calls' totals
    GraphvizArgs g{};
    std::vector<uint64_t> toff;

    // The labels come from the features: asked for behind the batch's checks, and uploaded (the handle's first graphviz call) before a context is leased.
    int after_batch_check(kgpu_dict *dict) { return require_features(dict, who); }
    int after_length_check(kgpu_dict *dict) { return ensure_label_pool(dict); }
    void begin() { text_offsets[0] = 0; }
    size_t chunk_words(uint64_t m) const { return (size_t)m + 1; }   // sent_len [m + 1]
    void fill(const LatticeChunk &f) {
        g = GraphvizArgs{};
        g.utf8 = f.utf8; g.offsets = f.offsets; g.n = f.m; g.arena = f.arena; g.desc = f.desc;
        g.conn = f.conn; g.conn_rows = f.conn_rows;
        g.label = d->label; g.label_off = d->label_off; g.n_morph = (uint32_t)d->info.n_morphs;
        g.full_state = full_state ? 1u : 0u; g.dpi = dpi;
        g.sent_len = f.words;
    }
    int measure(hipStream_t st) { return launch_graphviz_measure(g, st); }
    void totals(const uint64_t *t[2]) const { t[0] = g.sent_len + g.n; }   // the chunk's bytes
    bool fits(const uint64_t done[2], const uint64_t sz[2]) const { return done[0] + sz[0] <= text_capacity; }
    size_t out_bytes(const uint64_t sz[2]) const { return (size_t)sz[0]; }
    void place(uint8_t *blk, const uint64_t sz[2]) { g.text = blk; g.text_cap = sz[0]; }
    int write(hipStream_t st) { return launch_graphviz_write(g, st); }
    // The text and the offsets are delivered only while nothing has overflowed.
    hipError_t deliver(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits, const char *&what) {
        if (!fits) return hipSuccess;
        hipError_t e;
        toff.resize((size_t)f.m + 1);
        what = "D2H text";
        if ((e = d2h(text + done[0], g.text, (size_t)sz[0], f.stream)) != hipSuccess) return e;
        what = "D2H offsets";
        return d2h(toff.data(), g.sent_len, (size_t)(f.m + 1) * 8, f.stream);
    }
    void fix_up(const LatticeChunk &f, const uint64_t done[2], const uint64_t *, bool fits) {
        if (fits) for (uint64_t i = 0; i <= f.m; ++i) text_offsets[f.lo + i] = done[0] + toff[(size_t)i];
    }
    void report(const uint64_t done[2]) { if (n_bytes) *n_bytes = done[0]; }
    void too_small(const uint64_t done[2]) { set_error("text buffer too small: need %llu, capacity %llu", (unsigned long long)done[0], (unsigned long long)text_capacity); }
};

}  // namespace

extern "C" int kgpu_graphviz_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint64_t dpi, int full_state,
                                   uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    GraphvizOps ops;
    if (!d || !offsets || !text_offsets || (text_capacity && !text)) { set_error("%s: null argument", ops.who); return KGPU_ERR_INVALID_ARG; }
    ops.d = d; ops.dpi = dpi; ops.full_state = full_state; ops.text = text; ops.text_capacity = text_capacity; ops.text_offsets = text_offsets; ops.n_bytes = n_bytes;
    return lattice_call(ops, d, utf8, offsets, n, status);
}
