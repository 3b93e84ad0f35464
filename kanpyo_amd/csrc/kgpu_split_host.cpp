// kanpyo_amd/csrc/kgpu_split_host.cpp -- read_line + trim_end on the device (kgpu_split.hip) behind the C ABI.
//
// Owns: kgpu_split_lines_device / kgpu_ctx_sync_split (a block resident in HBM, on a context's stream); split_block (a raw block in host memory: one copy
// to the device, the split) and the source of chunks made of it (ChunkSource::block), which kgpu_count_text shares (kgpu_normalize_text: split_block alone);
// and kgpu_tokenize_text_lines / kgpu_tokenize_text_words, the text column's wrappers around text_lines (kgpu_host.cpp).
#include <vector>

#include "kgpu_runtime.h"

// The split on c->stream behind whatever is queued there.  The context's split_* members are its scratch: the tile aggregates, and what the carry
// kernel publishes ([0] lines, [1] packed bytes).
static int enqueue_split(kgpu_ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t *d_offsets, uint64_t offsets_capacity, const char *who) {
    SplitArgs a{};
    a.in = d_in; a.len = len; a.out = d_out; a.offsets = d_offsets; a.off_cap = offsets_capacity;
    a.ntiles = split_tiles(d_in, len);
    int rc;
    if ((rc = c->split_report.arm()) || (rc = c->split_agg.ensure(((size_t)a.ntiles + 1) * sizeof(SplitTile)))) return rc;
    a.agg = (SplitTile *)c->split_agg.p;
    a.host_ctl = c->split_report.dev();
    const hipError_t e = (hipError_t)launch_split_lines(a, c->stream);
    if (e != hipSuccess) { set_error("%s: split launch: %s", who, hipGetErrorString(e)); return KGPU_ERR_HIP; }
    return c->split_report.record(c->stream, offsets_capacity);
}

extern "C" int kgpu_split_lines_device(kgpu_ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t *d_offsets, uint64_t offsets_capacity) {
    const char *who = "kgpu_split_lines_device";
    if (!c || (len && (!d_in || !d_out)) || (offsets_capacity && !d_offsets)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (len >= (1ull << 32)) { set_error("%s: block of 4 GiB or more; split it", who); return KGPU_ERR_INVALID_ARG; }
    if (len && d_in < d_out + len && d_out < d_in + len) { set_error("%s: d_out overlaps d_in", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    return enqueue_split(c, d_in, len, d_out, d_offsets, offsets_capacity, who);
}

extern "C" int kgpu_ctx_sync_split(kgpu_ctx *c, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!c) { set_error("kgpu_ctx_sync_split: null ctx"); return KGPU_ERR_INVALID_ARG; }
    if (n_lines) *n_lines = 0;
    if (n_bytes) *n_bytes = 0;
    if (!c->split_report.pending) return KGPU_OK;
    HIPCHECK(hipSetDevice(c->dict->device));
    uint64_t h[2];   // [0] lines, [1] packed bytes
    if (int rc = c->split_report.wait(h)) return rc;
    const uint64_t lines = h[0];
    if (n_lines) *n_lines = lines;
    if (lines + 1 > c->split_report.cap) {
        set_error("kgpu_ctx_sync_split: offsets capacity %llu, need %llu", (unsigned long long)c->split_report.cap, (unsigned long long)(lines + 1));
        return KGPU_ERR_CAPACITY;
    }
    if (n_bytes) *n_bytes = h[1];
    return KGPU_OK;
}

// ONE copy of the raw block to the device, then the split; the offsets table is sized by a guess and grown to the count the device found
int kgpu::split_block(kgpu_ctx *sc, const uint8_t *text, uint64_t len, const char *WHO, std::vector<uint64_t> &off, uint64_t &lines) {
    int rc;
    uint64_t packed = 0;
    if ((rc = sc->split_raw.ensure((size_t)len + 16)) || (rc = sc->split_text.ensure((size_t)len + 16))) return rc;
    if (len && (rc = ctx_h2d(sc, sc->split_raw.p, text, (size_t)len, "H2D text block"))) return rc;
    for (uint64_t cap = len / 16 + 1024;;) {
        if ((rc = sc->split_off.ensure((size_t)cap * 8))) return rc;
        if ((rc = enqueue_split(sc, (const uint8_t *)sc->split_raw.p, len, (uint8_t *)sc->split_text.p, (uint64_t *)sc->split_off.p, cap, WHO))) return rc;
        rc = kgpu_ctx_sync_split(sc, &lines, &packed);
        if (rc == KGPU_ERR_CAPACITY) { cap = lines + 1; continue; }
        if (rc) return rc;
        break;
    }
    off.resize((size_t)lines + 1);
    if (hipMemcpy(off.data(), sc->split_off.p, (size_t)(lines + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H offsets failed", WHO); return KGPU_ERR_HIP; }
    return KGPU_OK;
}

// A raw block in host memory as the source of a chunked call: the copy and the split on a pooled context that owns the block, the packed lines and their
// offsets until the source goes; four chunks in flight, one pooled context each (the dictionary's shared streams run that many launches side by side).
int ChunkSource::block(kgpu_dict *d_, const char *who, const uint8_t *text, uint64_t len, bool features) {
    if (len >= (1ull << 32)) { set_error("%s: block of 4 GiB or more; split it", who); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if (features && (rc = require_features(d_, who))) return rc;
    HIPCHECK(hipSetDevice(d_->device));
    d = d_; depth = 4; held_back = 0; empty_chunk = false;
    if ((rc = split.get(d)) || (rc = split_block(split.c, text, len, who, split_off, n))) return rc;
    offsets = split_off.data();
    return KGPU_OK;
}

// ---- the text column's wrappers: text_lines (kgpu_host.cpp) over such a source -------------------------------------------------------------
extern "C" int kgpu_tokenize_text_lines(kgpu_dict *d, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets,
                                        uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    return text_lines(d, Renderer(), "kgpu_tokenize_text_lines", text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes);
}

extern "C" int kgpu_tokenize_text_words(kgpu_words *w, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets,
                                        uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!w) { set_error("kgpu_tokenize_text_words: null argument"); return KGPU_ERR_INVALID_ARG; }
    return text_lines(w->dict, Renderer(w), "kgpu_tokenize_text_words", text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes);
}
