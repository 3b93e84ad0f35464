// kanpyo_amd/csrc/kgpu_split_host.cpp -- read_line + trim_end on the device (kgpu_split.hip) behind the C ABI.
//
// Owns: kgpu_split_lines_device / kgpu_ctx_sync_split (a block resident in HBM, on a context's stream) and kgpu_tokenize_text_lines
// (a raw block in host memory: one copy to the device, the split, then the lines go through the launch chain and the render in chunks
// on pooled contexts -- their inputs are pointers into the split's output, nothing of the text returns to the host in between).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "kgpu_runtime.h"

// The split on c->stream behind whatever is queued there.  The context's split_* members are its scratch: the tile aggregates, the mapped words the
// carry kernel publishes ([0] lines, [1] packed bytes), the event behind the last launch.
static int enqueue_split(kgpu_ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t *d_offsets, uint64_t offsets_capacity, const char *who) {
    if (c->split_pending) { c->split_pending = false; HIPCHECK(hipEventSynchronize(c->split_ev)); }   // (its words are about to be reset)
    SplitArgs a{};
    a.in = d_in; a.len = len; a.out = d_out; a.offsets = d_offsets; a.off_cap = offsets_capacity;
    a.ntiles = split_tiles(d_in, len);
    int rc;
    if ((rc = c->split_agg.ensure(((size_t)a.ntiles + 1) * sizeof(SplitTile))) || (rc = c->split_ctl.ensure(16, true))) return rc;
    if (!c->split_ev) HIPCHECK(hipEventCreateWithFlags(&c->split_ev, hipEventDisableTiming));
    unsigned long long *h = (unsigned long long *)c->split_ctl.h;
    h[0] = 0; h[1] = 0;   // (this context's previous split has been synced)
    a.agg = (SplitTile *)c->split_agg.p;
    a.host_ctl = (unsigned long long *)c->split_ctl.d;
    const hipError_t e = (hipError_t)launch_split_lines(a, c->stream);
    if (e != hipSuccess) { set_error("%s: split launch: %s", who, hipGetErrorString(e)); return KGPU_ERR_HIP; }
    HIPCHECK(hipEventRecord(c->split_ev, c->stream));
    c->split_pending = true;
    c->split_cap = offsets_capacity;
    return KGPU_OK;
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
    if (!c->split_pending) return KGPU_OK;
    HIPCHECK(hipSetDevice(c->dict->device));
    c->split_pending = false;
    HIPCHECK(hipEventSynchronize(c->split_ev));
    const unsigned long long *h = (const unsigned long long *)c->split_ctl.h;
    const uint64_t lines = h[0];
    if (n_lines) *n_lines = lines;
    if (lines + 1 > c->split_cap) {
        set_error("kgpu_ctx_sync_split: offsets capacity %llu, need %llu", (unsigned long long)c->split_cap, (unsigned long long)(lines + 1));
        return KGPU_ERR_CAPACITY;
    }
    if (n_bytes) *n_bytes = h[1];
    return KGPU_OK;
}

// ---- kgpu_tokenize_text_lines: a raw block in host memory -> the CLI's output ---------------------------------------------------------
namespace {

// One chunk of the block's lines on a pooled context: lines [lo, lo + m) of the split's table.
struct TextJob {
    kgpu_ctx *c = nullptr;
    uint64_t lo = 0, m = 0;
};

struct TextCall {
    const uint8_t *d_text;        // the split's packed lines and their offsets, in the splitting context's device memory
    const uint64_t *d_off;
    const uint64_t *off;          // ... and the host's copy of the offsets
    uint8_t *text; uint64_t text_capacity; uint64_t *text_offsets; uint8_t *status;
    uint64_t text_done = 0;
    bool overflow = false;        // a caller's buffer is too small: from here on the chunks are only counted
};

const char *WHO = "kgpu_tokenize_text_lines";

// the buffers of ChunkBlock::prepare's `lines` form, without an input block: the chunk's input is where the split left it
int text_prepare(kgpu_ctx *c, uint64_t n, uint64_t total) {
    const uint64_t cap = total + n + 1;   // tokens <= chars + 1 <= bytes + 1 per sentence: never too small
    int rc;
    if ((rc = c->out_tok.ensure((size_t)cap * sizeof(kgpu_token) + 64)) || (rc = c->out_status.ensure((size_t)n + 16)) || (rc = c->out_off.ensure((size_t)(n + 1) * 8)) ||
        (rc = c->lines_off.ensure((size_t)(n + 1) * 8, true)) || (rc = c->lines_status.ensure((size_t)n + 16, true)) || (rc = c->lines_text.ensure((size_t)total * 16 + 4096, true)))
        return rc;
    return KGPU_OK;
}

int text_render(const TextCall &t, const TextJob &j) {
    kgpu_ctx *c = j.c;
    return enqueue_lines(c, t.d_text, t.d_off + j.lo, j.m, (const kgpu_token *)c->out_tok.p, (const uint64_t *)c->out_off.p, (uint8_t *)c->lines_text.d, c->lines_text.bytes,
                         (uint64_t *)c->lines_off.d, (const uint8_t *)c->out_status.p, (uint8_t *)c->lines_status.d, WHO);
}

int text_submit(const TextCall &t, const TextJob &j) {
    kgpu_ctx *c = j.c;
    const uint64_t total = t.off[j.lo + j.m] - t.off[j.lo];
    int rc;
    if ((rc = text_prepare(c, j.m, total))) return rc;
    if ((rc = tokenize_device_impl(c, t.d_text, t.d_off + j.lo, j.m, total, (kgpu_token *)c->out_tok.p, nullptr, nullptr, nullptr, nullptr, total + j.m + 1,
                                   (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p, WHO)))
        return rc;
    return text_render(t, j);
}

// (what pipe_finish_lines does for a chunk of kgpu_tokenize_batch_lines, kgpu_host.cpp)
int text_finish(TextCall &t, const TextJob &j) {
    kgpu_ctx *c = j.c;
    const auto reruns = [c] { return c->rt.window_reruns + c->rt.tail_reruns + c->rt.arena_regrows; };
    const uint64_t r0 = reruns();
    int rc = kgpu_ctx_sync(c, nullptr);
    if (rc) return rc;
    if (reruns() != r0 && (rc = text_render(t, j))) return rc;   // the chain ran again behind the render: the render once more
    uint64_t bytes = 0;
    rc = kgpu_ctx_sync_lines(c, &bytes);
    if (rc == KGPU_ERR_CAPACITY) {
        if ((rc = c->lines_text.ensure((size_t)bytes + 64, true)) || (rc = text_render(t, j))) return rc;
        rc = kgpu_ctx_sync_lines(c, &bytes);
    }
    if (rc) return rc;
    if (t.text_done + bytes > t.text_capacity) t.overflow = true;
    if (!t.overflow) {
        const uint64_t *toff = (const uint64_t *)c->lines_off.h;
        if (bytes) parallel_copy(t.text + t.text_done, c->lines_text.h, (size_t)bytes);
        for (uint64_t i = 0; i <= j.m; ++i) t.text_offsets[j.lo + i] = t.text_done + toff[i];
        if (t.status && j.m) std::memcpy(t.status + j.lo, c->lines_status.h, (size_t)j.m);
    }
    t.text_done += bytes;
    return KGPU_OK;
}

}  // namespace

extern "C" int kgpu_tokenize_text_lines(kgpu_dict *d, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets,
                                        uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!d || (len && !text) || (text_capacity && !out_text) || (offsets_capacity && !text_offsets) || !n_lines || !n_bytes) { set_error("%s: null argument", WHO); return KGPU_ERR_INVALID_ARG; }
    *n_lines = 0; *n_bytes = 0;
    if (len >= (1ull << 32)) { set_error("%s: block of 4 GiB or more; split it", WHO); return KGPU_ERR_INVALID_ARG; }
    {
        std::lock_guard<std::mutex> g(d->feat_mu);
        if (!d->feat) { set_error("%s: the dictionary has no feature tables: call kgpu_dict_set_features first", WHO); return KGPU_ERR_INVALID_ARG; }
    }
    HIPCHECK(hipSetDevice(d->device));
    workers().start();   // (parallel_copy's helpers; none to be had: it copies on this thread)
    kgpu_ctx *sc = nullptr;   // the splitting context: it owns the block, the packed lines and their offsets until the call is over
    int rc = pool_get(d, &sc);
    if (rc) return rc;
    constexpr int DEPTH = 4;   // chunks in flight, one pooled context each (the dictionary's shared streams run that many launches side by side)
    TextJob jobs[DEPTH];
    std::vector<uint64_t> off;
    uint64_t lines = 0, packed = 0;
    const auto give_back = [&](int r) {
        sc->h2d_queued = false;
        pool_put(d, sc);
        for (TextJob &j : jobs) if (j.c) pool_put(d, j.c);
        return r;
    };
    // ONE copy of the raw block to the device, then the split; the offsets table is sized by a guess and grown to the count the device found
    if ((rc = sc->split_raw.ensure((size_t)len + 16)) || (rc = sc->split_text.ensure((size_t)len + 16))) return give_back(rc);
    if (len && (rc = ctx_h2d(sc, sc->split_raw.p, text, (size_t)len, "H2D text block"))) return give_back(rc);
    for (uint64_t cap = len / 16 + 1024;;) {
        if ((rc = sc->split_off.ensure((size_t)cap * 8))) return give_back(rc);
        if ((rc = enqueue_split(sc, (const uint8_t *)sc->split_raw.p, len, (uint8_t *)sc->split_text.p, (uint64_t *)sc->split_off.p, cap, WHO))) return give_back(rc);
        rc = kgpu_ctx_sync_split(sc, &lines, &packed);
        if (rc == KGPU_ERR_CAPACITY) { cap = lines + 1; continue; }
        if (rc) return give_back(rc);
        break;
    }
    off.resize((size_t)lines + 1);
    if (hipMemcpy(off.data(), sc->split_off.p, (size_t)(lines + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) { set_error("%s: D2H offsets failed", WHO); return give_back(KGPU_ERR_HIP); }
    *n_lines = lines;
    TextCall t{(const uint8_t *)sc->split_text.p, (const uint64_t *)sc->split_off.p, off.data(), out_text, text_capacity, text_offsets, status};
    t.overflow = lines + 1 > offsets_capacity;
    if (!t.overflow) text_offsets[0] = 0;
    // the chunk sizes of the large host calls (run_pipeline, kgpu_host.cpp)
    const TestHooks hooks = test_hooks();
    const uint64_t CHUNK_BYTES = std::min<uint64_t>(hooks.chunk_bytes, 2ull << 20);
    const uint64_t CHUNK_SENTS = std::min<uint64_t>(hooks.chunk_sents, std::min<uint64_t>(8192, std::max<uint64_t>(1024, lines / 12)));
    uint64_t done = 0;
    int head = 0, inflight = 0;   // jobs[head .. head + inflight) (mod DEPTH) are active, oldest first
    while (!rc && done < lines) {
        if (inflight == DEPTH) {
            rc = text_finish(t, jobs[head]);
            head = (head + 1) % DEPTH; --inflight;
            if (rc) break;
        }
        TextJob &j = jobs[(head + inflight) % DEPTH];
        if (!j.c && (rc = pool_get(d, &j.c))) break;
        uint64_t m = 0;
        while (done + m < lines && m < CHUNK_SENTS && (m == 0 || off[done + m + 1] - off[done] <= CHUNK_BYTES)) ++m;
        j.lo = done; j.m = m;
        if ((rc = text_submit(t, j))) {   // (a batch may be queued without its render: the context goes back to the pool idle)
            if (j.c->pending) (void)kgpu_ctx_sync(j.c, nullptr);
            break;
        }
        ++inflight;
        done += m;
    }
    while (inflight) {   // drain in order (also after an error: the contexts go back to the pool idle)
        const int r2 = text_finish(t, jobs[head]);
        if (!rc) rc = r2;
        head = (head + 1) % DEPTH; --inflight;
    }
    *n_bytes = t.text_done;
    if (rc) return give_back(rc);
    if (t.overflow) {
        set_error("%s: buffers too small: need %llu text bytes (capacity %llu) and %llu offsets (capacity %llu)", WHO, (unsigned long long)t.text_done,
                  (unsigned long long)text_capacity, (unsigned long long)(lines + 1), (unsigned long long)offsets_capacity);
        return give_back(KGPU_ERR_CAPACITY);
    }
    return give_back(KGPU_OK);
}
