// kanpyo_amd/csrc/kgpu_split_host.cpp -- read_line + trim_end on the device (kgpu_split.hip) behind the C ABI.
//
// Owns: kgpu_split_lines_device / kgpu_ctx_sync_split (a block resident in HBM, on a context's stream) and kgpu_tokenize_text_lines /
// kgpu_tokenize_text_words (one body, text_lines: a raw block in host memory: one copy to the device, the split, then the lines go through the launch chain and the render in chunks
// on pooled contexts -- their inputs are pointers into the split's output, nothing of the text returns to the host in between; the
// chunks are LinesChunk in run_pipeline, kgpu_runtime.h, as those of kgpu_tokenize_batch_lines); split_block, the copy and the split in front of them, which
// kgpu_count_text (kgpu_count_host.cpp) shares.
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

// ---- kgpu_tokenize_text_lines: a raw block in host memory -> the CLI's output ---------------------------------------------------------
// One chunk of the block's lines on a pooled context: lines [lo, lo + m) of the split's table, whose input is where the split left it.
struct TextJob {
    kgpu_ctx *c = nullptr;
    uint64_t lo = 0, m = 0;
    LinesChunk out;
};

// kgpu_tokenize_text_lines (words and vocab null), kgpu_tokenize_text_words and kgpu_encode_text: the chunks differ in their renderer alone.
int kgpu::text_lines(kgpu_dict *d, const kgpu_words *words, const kgpu_vocab *vocab, const char *WHO, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                      uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!d || (len && !text) || (text_capacity && !out_text) || (offsets_capacity && !text_offsets) || !n_lines || !n_bytes) { set_error("%s: null argument", WHO); return KGPU_ERR_INVALID_ARG; }
    *n_lines = 0; *n_bytes = 0;
    if (len >= (1ull << 32)) { set_error("%s: block of 4 GiB or more; split it", WHO); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = require_features(d, WHO))) return rc;
    HIPCHECK(hipSetDevice(d->device));
    kgpu_ctx *sc = nullptr;   // the splitting context: it owns the block, the packed lines and their offsets until the call is over
    if ((rc = pool_get(d, &sc))) return rc;
    constexpr int DEPTH = 4;   // chunks in flight, one pooled context each (the dictionary's shared streams run that many launches side by side)
    std::vector<uint64_t> off;
    uint64_t lines = 0;
    const auto give_back = [&](int r) {
        sc->h2d_queued = false;
        pool_put(d, sc);
        return r;
    };
    if ((rc = split_block(sc, text, len, WHO, off, lines))) return give_back(rc);
    *n_lines = lines;
    const uint8_t *d_text = (const uint8_t *)sc->split_text.p;   // the chunks' input: pointers into the split's output
    const uint64_t *d_off = (const uint64_t *)sc->split_off.p;
    LinesSink sink{out_text, text_capacity, text_offsets, status, false};   // (status is bounded by offsets_capacity: nothing of it after an overflow)
    if (vocab) sink.unit = 4;
    sink.overflow = lines + 1 > offsets_capacity;
    if (!sink.overflow) text_offsets[0] = 0;
    rc = run_pipeline<TextJob>(d, off.data(), lines, DEPTH, 0, false, nullptr,
        [&](TextJob &j) {
            j.out.words = words; j.out.vocab = vocab;
            const int r = j.out.prepare(j.c, j.m, off[j.lo + j.m] - off[j.lo]);
            return r ? r : j.out.launch(j.c, d_text, d_off + j.lo, WHO);
        },
        [&](TextJob &j) { return j.out.finish(j.c, j.lo, sink, WHO); });
    *n_bytes = sink.text_done;
    if (rc) return give_back(rc);
    if (sink.overflow) {
        set_error("%s: buffers too small: need %llu text bytes (capacity %llu) and %llu offsets (capacity %llu)", WHO, (unsigned long long)sink.text_done,
                  (unsigned long long)text_capacity, (unsigned long long)(lines + 1), (unsigned long long)offsets_capacity);
        return give_back(KGPU_ERR_CAPACITY);
    }
    return give_back(KGPU_OK);
}

extern "C" int kgpu_tokenize_text_lines(kgpu_dict *d, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets,
                                        uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    return text_lines(d, nullptr, nullptr, "kgpu_tokenize_text_lines", text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes);
}

extern "C" int kgpu_tokenize_text_words(kgpu_words *w, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets,
                                        uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!w) { set_error("kgpu_tokenize_text_words: null argument"); return KGPU_ERR_INVALID_ARG; }
    return text_lines(w->dict, w, nullptr, "kgpu_tokenize_text_words", text, len, out_text, text_capacity, text_offsets, offsets_capacity, status, n_lines, n_bytes);
}
