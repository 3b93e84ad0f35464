// kanpyo_amd/csrc/kgpu_host.cpp -- kgpu_tokenize_batch beyond the small calls: the large-call pipeline over host buffers.
//
// Owns: the worker pool (with no threads its tasks run on the calling thread), parallel_copy, is_pinned_host, the argument check of a
// host batch, a chunk's input block (ChunkInput) and mapped result block (ChunkBlock, shared with kgpu_multi.cpp), the chunk sizes of the
// pipeline (the ring itself is run_pipeline, kgpu_runtime.h), the 24-byte per-chunk fallback for tokens beyond the 8-byte record (HostJob),
// kgpu_tokenize_batch; the frame of the other chunked host calls -- a chunk's records (RecordsChunk), its render (LinesChunk) by one of three
// renderers (Renderer), a packed batch as a source of chunks (ChunkSource::packed, ::stage) -- with the body of the lines / words / encode calls over a
// source and a renderer (lines_call) and its two wrappers (batch_lines, text_lines: the argument checks, the sink and the message of each column), kgpu_tokenize_batch_lines / _words; and kgpu_host_alloc / kgpu_host_free.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <mutex>
#include <thread>
#include <pthread.h>
#include <vector>

#include "kgpu_runtime.h"

// ---- the 24-byte form of one chunk ----------------------------------------------------------------------
// What a chunk of a large call falls back to when a token does not fit the 8-byte record (pipe_finish): 24-byte records on the
// device, device-to-host copies on the context's stream.
struct HostJob {
    kgpu_ctx *c = nullptr;
    uint64_t lo = 0, m = 0;        // sentences [lo, lo + m) of the call
    std::vector<uint64_t> rel;     // chunk-relative byte offsets (must outlive the asynchronous H2D copy)
};

static int host_job_submit(HostJob &j, const uint8_t *utf8, const uint64_t *offsets) {
    kgpu_ctx *c = j.c;
    const uint64_t *off = offsets + j.lo;
    const uint64_t n = j.m, base = off[0], total = off[n] - base;
    j.rel.resize((size_t)n + 1);
    for (uint64_t i = 0; i <= n; ++i) j.rel[(size_t)i] = off[i] - base;
    const uint64_t cap = token_bound(total, n);
    int rc;
    if ((rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure((size_t)(n + 1) * 8)) ||
        (rc = c->out_tok.ensure((size_t)cap * sizeof(kgpu_token) + 64)) ||
        (rc = c->out_off.ensure((size_t)(n + 1) * 8)) || (rc = c->out_status.ensure((size_t)n + 16)))
        return rc;
    if ((total && (rc = ctx_h2d(c, c->in_utf8.p, utf8 + base, (size_t)total, "H2D utf8"))) ||
        (rc = ctx_h2d(c, c->in_off.p, j.rel.data(), (size_t)(n + 1) * 8, "H2D offsets")))
        return rc;
    return kgpu_tokenize_device(c, (const uint8_t *)c->in_utf8.p, (const uint64_t *)c->in_off.p, n, total,
                                (kgpu_token *)c->out_tok.p, cap, (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p);
}

// Wait for the job, copy its results behind the `tok_done` tokens already delivered (or only count, once the
// caller's buffer has overflowed) and make the chunk-local token offsets global.
static int host_job_finish(HostJob &j, kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, uint8_t *status,
                           uint64_t &tok_done, bool &overflow) {
    kgpu_ctx *c = j.c;
    uint64_t got = 0;
    int rc = kgpu_ctx_sync(c, &got);
    if (rc) return rc;
    if (tok_done + got > token_capacity) overflow = true;
    hipError_t e;
    if (!overflow) {
        if (got && (e = hipMemcpyAsync(tokens + tok_done, c->out_tok.p, (size_t)got * sizeof(kgpu_token), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) { set_error("D2H tokens: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
        if ((e = hipMemcpyAsync(tok_offsets + j.lo, c->out_off.p, (size_t)(j.m + 1) * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) { set_error("D2H offsets: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    }
    if (status && j.m && (e = hipMemcpyAsync(status + j.lo, c->out_status.p, (size_t)j.m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) { set_error("D2H status: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    // pageable destinations make these copies synchronous; pinned ones (kgpu_host_alloc) run at DMA speed while the
    // next chunks' kernels execute.  The offsets fix-up below needs the data, so wait for this stream's copies here.
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) { set_error("D2H sync: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    if (!overflow) for (uint64_t i = 0; i <= j.m; ++i) tok_offsets[j.lo + i] += tok_done;  // chunk-local -> global
    tok_done += got;
    return KGPU_OK;
}

// ---- large host calls: 8-byte records over PCIe, expanded by a few host threads ---------------------------
// What a large call moves device -> host is 24 bytes per token, seven times its input (32 tokens per 113-byte sentence on the
// cfg 2 corpus): ~65 M sentences/s at PCIe speed, and through pageable destinations far less.  Here the compaction kernel writes
// 8-byte kgpu_token8 records straight into pinned, device-mapped host memory (its stores are the transfer: no copy node, no
// D2H call), and worker threads expand them into the caller's 24-byte records (any memory: the expansion replaces the copy
// a pageable destination costs anyway) while the next chunks compute.
namespace kgpu {
// A few host threads for the large calls: expansion of the 8-byte records, staging copies.  Heap-allocated and never destroyed (its
// threads end with the process).  fork(): the child has none of the parent's threads, and its copy of the pool may hold a locked mutex
// or a condition variable with waiters -- the child handler abandons it and the first use there makes a fresh one.  Thread creation
// can fail (std::system_error): start() reports how many threads run, and with none submit() runs every task on the calling thread
// (every counter a caller waits on is set before its tasks are submitted, so wait_zero then returns at once).
unsigned WorkerPool::start() {
    std::lock_guard<std::mutex> g(mu);
    if (!th.empty()) return (unsigned)th.size();
    unsigned n = 0;
    if (const char *e = getenv("KGPU_HOST_THREADS")) n = (unsigned)atoi(e);
    if (n == 0) n = std::min(8u, std::max(2u, std::thread::hardware_concurrency() / 8));
    for (unsigned i = 0; i < n; ++i) {
        try {
            th.emplace_back([this] {
                for (;;) {
                    std::function<void()> f;
                    { std::unique_lock<std::mutex> l(mu); cv.wait(l, [this] { return !q.empty(); }); f = std::move(q.front()); q.pop_front(); }
                    f();
                }
            });
        } catch (...) { break; }  // out of threads: run with what there is
    }
    return (unsigned)th.size();
}
void WorkerPool::submit(std::function<void()> f) {
    bool queued;
    { std::lock_guard<std::mutex> g(mu); queued = !th.empty(); if (queued) q.push_back(std::move(f)); }
    if (queued) cv.notify_one();
    else f();   // no worker threads: the caller's own
}
// A counter of tasks reaching zero: a short spin (the common case: the workers are almost through), then sleeps on the pool's
// completion signal instead of burning a core the workers could use.
void WorkerPool::wait_zero(std::atomic<int> &counter) {
    // (the tasks waited for here are tens of microseconds long: a sleep costs more than it saves until the wait has lasted a while)
    timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {
        for (int spin = 0; spin < 64; ++spin) { if (counter.load(std::memory_order_acquire) == 0) return; std::this_thread::yield(); }
        timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((t1.tv_sec - t0.tv_sec) * 1000000ll + (t1.tv_nsec - t0.tv_nsec) / 1000 > 2000) break;
    }
    std::unique_lock<std::mutex> l(done_mu);
    while (counter.load(std::memory_order_acquire) != 0) done_cv.wait_for(l, std::chrono::microseconds(200));
}
void WorkerPool::task_done(std::atomic<int> &counter) {
    if (counter.fetch_sub(1, std::memory_order_acq_rel) == 1) { std::lock_guard<std::mutex> g(done_mu); done_cv.notify_all(); }
}
static std::atomic<WorkerPool *> g_pool{nullptr};
static std::atomic<int> g_pool_lock{0};
static void pool_atfork_child() { g_pool.store(nullptr, std::memory_order_relaxed); g_pool_lock.store(0, std::memory_order_relaxed); }
WorkerPool &workers() {
    WorkerPool *w = g_pool.load(std::memory_order_acquire);
    if (w) return *w;
    while (g_pool_lock.exchange(1, std::memory_order_acquire)) std::this_thread::yield();
    static bool hooked = false;
    if (!hooked) { hooked = true; pthread_atfork(nullptr, nullptr, pool_atfork_child); }
    w = g_pool.load(std::memory_order_relaxed);
    if (!w) { w = new WorkerPool(); g_pool.store(w, std::memory_order_release); }
    g_pool_lock.store(0, std::memory_order_release);
    return *w;
}
}  // namespace kgpu

// The layout of a chunk's input block (kgpu_runtime.h: ChunkInput) and the context's buffers big enough for it.
int ChunkInput::prepare(kgpu_ctx *c, uint64_t n_, uint64_t total_, bool staged) {
    n = n_; total = total_;
    in_off = ((size_t)(n + 1) * 8 + 63) & ~(size_t)63;
    const size_t in_bytes = in_off + (size_t)total + 16;
    int rc;
    if ((rc = c->in_block.ensure(in_bytes)) || (staged && (rc = c->pin_in.ensure(in_bytes, false)))) return rc;
    return KGPU_OK;
}
// ... and of its mapped result block (ChunkBlock)
int ChunkBlock::prepare(kgpu_ctx *c, uint64_t n, uint64_t total, bool staged) {
    cap = token_bound(total, n);
    off_first = ((size_t)cap * 8 + 63) & ~(size_t)63;
    off_toff = off_first + (((size_t)n * 8 + 63) & ~(size_t)63);
    off_status = off_toff + (((size_t)(n + 1) * 8 + 63) & ~(size_t)63);
    int rc;
    if ((rc = in.prepare(c, n, total, staged)) || (rc = c->pin_out.ensure(off_status + (size_t)n + 64, true)) || (rc = c->out_status.ensure((size_t)n + 16)) ||
        (rc = c->out_off.ensure((size_t)(n + 1) * 8)))
        return rc;
    return KGPU_OK;
}
// The launch chain over the input block (its offsets start at `base`), 8-byte records into the mapped block.
int ChunkBlock::launch(kgpu_ctx *c, uint64_t base, const char *who) const {
    uint8_t *po = (uint8_t *)c->pin_out.d;
    return tokenize_device_impl(c, in.d_text(c, base), in.d_offsets(c), in.n, in.total, nullptr, (kgpu_token8 *)po, (uint32_t *)(po + off_first), po + off_status,
                                (uint64_t *)(po + off_toff), cap, (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p, who);
}
MergeSrc ChunkBlock::results(const kgpu_ctx *c) const {
    const uint8_t *ph = (const uint8_t *)c->pin_out.h;
    return MergeSrc{(const kgpu_token8 *)ph, (const uint32_t *)(ph + off_first), (const uint64_t *)(ph + off_toff), ph + off_status};
}

// ---- one chunk of a chunked host call (kgpu_runtime.h: RecordsChunk, LinesChunk, Renderer) ------------------
int RecordsChunk::prepare(kgpu_ctx *c, uint64_t n_, uint64_t total_) {
    n = n_; total = total_;
    int rc;
    if ((rc = c->out_tok.ensure((size_t)token_bound(total, n) * sizeof(kgpu_token) + 64)) || (rc = c->out_status.ensure((size_t)n + 16)) ||
        (rc = c->out_off.ensure((size_t)(n + 1) * 8)) || (rc = c->lines_status.ensure((size_t)n + 16, true)))
        return rc;
    return KGPU_OK;
}
// The launch chain over the chunk's input where it lies in device memory, 24-byte records into HBM.
int RecordsChunk::launch(kgpu_ctx *c, const char *who) const {
    return tokenize_device_impl(c, d_utf8, d_offsets, n, total, (kgpu_token *)c->out_tok.p, nullptr, nullptr, nullptr, nullptr, token_bound(total, n),
                                (uint64_t *)c->out_off.p, (uint8_t *)c->out_status.p, who);
}
DeviceRecords RecordsChunk::records(const kgpu_ctx *c) const {
    return DeviceRecords{d_utf8, d_offsets, n, (const kgpu_token *)c->out_tok.p, (const uint64_t *)c->out_off.p, (const uint8_t *)c->out_status.p, (uint8_t *)c->lines_status.d};
}

// The three renderers.  LINES: the text block starts at 16 bytes per input byte -- cfg 2 renders about 14.  WORDS: a surface line is at most the input's
// bytes and a byte per token, and a byte for the sentence; a field's names may be longer.  IDS: 4 bytes per kept token and bos / eos -- cfg 2 has a token
// per 3.6 bytes.  LinesChunk::finish grows the block when a chunk's output outgrows the guess.
size_t Renderer::first_bytes(uint64_t total, uint64_t n) const {
    return kind == IDS ? ((size_t)total / 2 + (size_t)n * 2 + 1024) * 4 : kind == WORDS ? (size_t)total * 2 + (size_t)n + 4096 : (size_t)total * 16 + 4096;
}
int Renderer::enqueue(kgpu_ctx *c, const DeviceRecords &r, void *d_out, size_t out_bytes, uint64_t *d_off, const char *who) const {
    if (kind == IDS) return enqueue_encode(c, vocab, r, (int32_t *)d_out, out_bytes / 4, 0, 0, d_off, who);
    if (kind == WORDS) return enqueue_words(c, words, r, (uint8_t *)d_out, out_bytes, d_off, who);
    return enqueue_lines(c, r, (uint8_t *)d_out, out_bytes, d_off, who);
}

int LinesChunk::prepare(kgpu_ctx *c, uint64_t n_, uint64_t total_) {
    int rc;   // (the mapped blocks are allocated in the order offsets, status, text)
    if ((rc = c->lines_off.ensure((size_t)(n_ + 1) * 8, true)) || (rc = RecordsChunk::prepare(c, n_, total_)) || (rc = c->lines_text.ensure(renderer.first_bytes(total, n), true))) return rc;
    return KGPU_OK;
}
int LinesChunk::launch(kgpu_ctx *c, const char *who) const {
    const int rc = RecordsChunk::launch(c, who);
    return rc ? rc : render(c, who);
}
// The chunk's lines into the context's mapped blocks: text, chunk-relative text offsets, status.
int LinesChunk::render(kgpu_ctx *c, const char *who) const {
    return renderer.enqueue(c, records(c), c->lines_text.d, c->lines_text.bytes, (uint64_t *)c->lines_off.d, who);
}
// Wait for the chunk's render (its text is in the context's mapped block then) and copy the text behind the bytes already delivered (or only count,
// once a buffer of the caller's has overflowed).  A rerun of the chunk's chain inside kgpu_ctx_sync came after the render queued behind the first
// pass: the render once more; a text block too small for the chunk: a bigger one and the render once more.
int LinesChunk::finish(kgpu_ctx *c, uint64_t lo, LinesSink &s, const char *who) const {
    const auto reruns = [c] { return c->rt.window_reruns + c->rt.tail_reruns + c->rt.arena_regrows; };
    const uint64_t r0 = reruns();
    int rc = kgpu_ctx_sync(c, nullptr);   // (24-byte records with capacity token_bound: never too small)
    if (rc) return rc;
    if (reruns() != r0 && (rc = render(c, who))) return rc;
    uint64_t bytes = 0;   // (elements of s.unit bytes)
    rc = kgpu_ctx_sync_lines(c, &bytes);
    if (rc == KGPU_ERR_CAPACITY) {
        if ((rc = c->lines_text.ensure((size_t)(bytes * s.unit) + 64, true)) || (rc = render(c, who))) return rc;
        rc = kgpu_ctx_sync_lines(c, &bytes);
    }
    if (rc) return rc;
    if (s.text_done + bytes > s.text_capacity) s.overflow = true;
    if (!s.overflow) {
        const uint64_t *toff = (const uint64_t *)c->lines_off.h;
        if (bytes) parallel_copy(s.text + s.text_done * s.unit, c->lines_text.h, (size_t)(bytes * s.unit));
        for (uint64_t i = 0; i <= n; ++i) s.text_offsets[lo + i] = s.text_done + toff[i];
    }
    if (s.status && n && (!s.overflow || s.status_after_overflow)) std::memcpy(s.status + lo, c->lines_status.h, (size_t)n);
    s.text_done += bytes;
    return KGPU_OK;
}

struct PipeJob {
    kgpu_ctx *c = nullptr;
    uint64_t lo = 0, m = 0;
    ChunkBlock blk;                                     // its input block and mapped result block
    std::atomic<int> tasks{0};                          // expansion tasks still reading pin_out
    bool stream = false;                                // the call is large: its 24-byte records are written with non-temporal stores (kgpu_runtime.h: expand_tokens)
};

// memcpy of a large block with the workers' help (the calling thread's staging copy is what limits a large call otherwise)
void kgpu::parallel_copy(void *dst, const void *src, size_t bytes) {
    constexpr size_t PIECE = 256 * 1024;
    if (bytes < 2 * PIECE) { std::memcpy(dst, src, bytes); return; }
    const size_t np = std::min<size_t>(8, bytes / PIECE), each = ((bytes + np - 1) / np + 63) & ~(size_t)63;  // np * each >= bytes (rounded UP: a floor here lost the last bytes of a chunk)
    std::atomic<int> left{(int)np - 1};
    for (size_t k = 1; k < np; ++k) {
        const size_t lo = k * each, hi = std::min(bytes, lo + each);
        std::atomic<int> *l = &left;
        workers().submit([=] { if (hi > lo) std::memcpy((uint8_t *)dst + lo, (const uint8_t *)src + lo, hi - lo); workers().task_done(*l); });
    }
    std::memcpy(dst, src, std::min(bytes, each));
    workers().wait_zero(left);
}

bool kgpu::is_pinned_host(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// The chunk's input goes to the device as ONE block [offsets (absolute, as the caller has them) | bytes]; the kernels subtract
// offsets[0] themselves, the text pointer is biased by it.  Pinned caller memory is copied from directly (DMA), pageable memory through
// the context's pinned staging block, filled with the workers' help.  off: the chunk's first offset.
int kgpu::upload_input(kgpu_ctx *c, const ChunkInput &in, const uint8_t *utf8, const uint64_t *off, bool pinned_in) {
    uint8_t *dblk = (uint8_t *)c->in_block.p;
    const uint64_t n = in.n, base = off[0], total = in.total;
    int rc;
    if (pinned_in) {
        if ((rc = ctx_h2d(c, dblk, off, (size_t)(n + 1) * 8, "H2D input")) ||
            (total && (rc = ctx_h2d(c, dblk + in.in_off, utf8 + base, (size_t)total, "H2D input"))))
            return rc;
    } else {
        std::memcpy(c->pin_in.h, off, (size_t)(n + 1) * 8);
        if (total) parallel_copy((uint8_t *)c->pin_in.h + in.in_off, utf8 + base, (size_t)total);
        if ((rc = ctx_h2d(c, dblk, c->pin_in.h, in.in_off + (size_t)total, "H2D input block"))) return rc;
    }
    return KGPU_OK;
}

static int pipe_submit(PipeJob &j, const uint8_t *utf8, const uint64_t *offsets, bool pinned_in) {
    kgpu_ctx *c = j.c;
    workers().wait_zero(j.tasks);  // the block's previous results are still being expanded
    const uint64_t *off = offsets + j.lo;
    int rc;
    if ((rc = j.blk.prepare(c, j.m, off[j.m] - off[0], !pinned_in)) || (rc = upload_input(c, j.blk.in, utf8, off, pinned_in))) return rc;
    return j.blk.launch(c, off[0], "kgpu_tokenize_batch");
}

// Wait for the chunk's kernels (its records are in host memory then), hand the expansion to the workers in slices of 2048 sentences.
static int pipe_finish(PipeJob &j, const uint8_t *utf8, const uint64_t *offsets, kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets,
                       uint8_t *status, uint64_t &tok_done, bool &overflow, std::atomic<int> &outstanding) {
    kgpu_ctx *c = j.c;
    uint64_t got = 0;
    int rc = kgpu_ctx_sync(c, &got);
    if (rc == KGPU_ERR_CAPACITY && c->h_ctl->pack_overflow) {  // a token beyond the 8-byte packing: this chunk once more, 24-byte records, the plain way
        // (the previous chunk's last expansion slice stores tok_offsets[j.lo] too -- the boundary entry -- and host_job_finish copies and then adds
        // to it: wait for the expansions in flight first)
        workers().wait_zero(outstanding);
        HostJob hj;
        hj.c = c; hj.lo = j.lo; hj.m = j.m;
        if ((rc = host_job_submit(hj, utf8, offsets))) return rc;
        return host_job_finish(hj, tokens, token_capacity, tok_offsets, status, tok_done, overflow);
    }
    if (rc) return rc;
    if (tok_done + got > token_capacity) overflow = true;
    const uint64_t tok_base = tok_done;
    tok_done += got;
    const MergeSrc r = j.blk.results(c);
    const kgpu_token8 *rec = r.rec;
    const uint32_t *first = r.first;
    const uint64_t *toff = r.toff;
    const uint8_t *st = r.st;
    const uint64_t SLICE = std::min<uint64_t>(2048, std::max<uint64_t>(256, j.m / 8));  // (a lone 4096-sentence call: eight slices, not two)
    const int nt = (int)((j.m + SLICE - 1) / SLICE);
    if (nt == 0) { if (!overflow) tok_offsets[j.lo] = tok_base; return KGPU_OK; }
    j.tasks.store(nt, std::memory_order_release);
    outstanding.fetch_add(nt, std::memory_order_acq_rel);
    const bool ovf = overflow, jstream = j.stream;
    const uint64_t lo = j.lo, m = j.m;
    for (int t = 0; t < nt; ++t) {
        const uint64_t a = (uint64_t)t * SLICE, b = std::min(m, a + SLICE);
        std::atomic<int> *jt = &j.tasks, *out = &outstanding;
        workers().submit([=] {
            if (!ovf) {
                const bool stream = jstream;
                expand_tokens(rec + toff[a], toff + a, first + 2 * a, b - a, tokens + tok_base + toff[a], stream);
                for (uint64_t i = a; i < b; ++i) tok_offsets[lo + i] = tok_base + toff[i];
                if (b == m) tok_offsets[lo + m] = tok_base + toff[m];
                if (stream) expand_fence();
            }
            if (status) std::memcpy(status + lo + a, st + a, (size_t)(b - a));
            workers().task_done(*jt);
            workers().task_done(*out);
        });
    }
    return KGPU_OK;
}

// The chunk sizes of a call of n sentences (run_pipeline, kgpu_runtime.h).
ChunkLimits kgpu::chunk_limits(uint64_t n) {
    const TestHooks hooks = test_hooks();
    // chunks of 8192 sentences, ten in the device pipeline (measured on 400k sentences: 16384 x 6: 55.6, 8192 x 10: 61.2, 4096 x 14: 58.8 M sentences/s)
    return ChunkLimits{std::min<uint64_t>(hooks.chunk_bytes, 2ull << 20),
                       std::min<uint64_t>(hooks.chunk_sents, std::min<uint64_t>(8192, std::max<uint64_t>(1024, n / 12)))};   // (round 6: the floor was 2048 -- with the pool kernel at 59 us per 4096 sentences a 4096-sentence call runs 182 -> 174 us as four chunks)
}
// The ring of kgpu_tokenize_batch / kgpu_tokenize_batch_lines; two of its jobs stay out of the device pipeline: their blocks are being expanded.
int kgpu::batch_depth() { return (int)std::min<uint64_t>(MAX_PIPE_DEPTH, std::max<uint64_t>(3, test_hooks().depth)); }
bool kgpu::batch_is_pinned(const uint8_t *utf8, const uint64_t *offsets, uint64_t n) { return (offsets[n] - offsets[0]) != 0 && is_pinned_host(utf8) && is_pinned_host(offsets); }

int kgpu::check_host_batch(const char *who, const uint64_t *offsets, uint64_t n, const uint8_t *utf8) {
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) { set_error("%s: offsets not monotone at %llu", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    if (offsets[n] - offsets[0] && !utf8) { set_error("%s: null utf8", who); return KGPU_ERR_INVALID_ARG; }
    return KGPU_OK;
}

extern "C" int kgpu_tokenize_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                   kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets,
                                   uint8_t *status, uint64_t *n_tokens) {
    if (!d || !offsets || !tok_offsets || (token_capacity && !tokens)) {
        set_error("kgpu_tokenize_batch: null argument");
        return KGPU_ERR_INVALID_ARG;
    }
    if (int rc = check_host_batch("kgpu_tokenize_batch", offsets, n, utf8)) return rc;
    const uint64_t kd0 = small_trace_on() ? cpu_ns() : 0;
    HIPCHECK(hipSetDevice(d->device));
    if (kd0) g_sc[11] += cpu_ns() - kd0;   // (KGPU_SMALL_TRACE: the CPU time of hipSetDevice)

    {
        const int rc = tokenize_small(d, utf8, offsets, n, tokens, token_capacity, tok_offsets, status, n_tokens);
        if (rc != -1) return rc;  // -1: not a small call, or a sentence needs a kernel that path does not launch: take the general path below
    }

    std::atomic<int> outstanding{0};
    uint64_t tok_done = 0;
    bool overflow = false;
    tok_offsets[0] = 0;
    const bool pinned_in = batch_is_pinned(utf8, offsets, n);
    const bool stream = expand_stream_wanted((uint64_t)n * 2);   // by the CALL's size (32 768 tokens ~ 16 384 sentences and more): a 4096-sentence call's records are read back at once
    const int rc = run_pipeline<PipeJob>(d, offsets, n, batch_depth(), 2, true, &outstanding,
        [&](PipeJob &j) { j.stream = stream; return pipe_submit(j, utf8, offsets, pinned_in); },
        [&](PipeJob &j) { return pipe_finish(j, utf8, offsets, tokens, token_capacity, tok_offsets, status, tok_done, overflow, outstanding); });
    if (n_tokens) *n_tokens = tok_done;
    if (!rc && overflow) {
        set_error("token buffer too small: need %llu, capacity %llu", (unsigned long long)tok_done, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return rc;
}

// A packed batch in host memory as the source of a chunked call: the ring of kgpu_tokenize_batch, two jobs held back.
int ChunkSource::packed(kgpu_dict *d_, const char *who, const uint8_t *utf8_, const uint64_t *offsets_, uint64_t n_, bool features, bool empty_chunk_) {
    int rc;
    if ((rc = check_host_batch(who, offsets_, n_, utf8_)) || (features && (rc = require_features(d_, who)))) return rc;
    HIPCHECK(hipSetDevice(d_->device));
    d = d_; offsets = offsets_; n = n_; utf8 = utf8_;
    depth = batch_depth(); held_back = 2; empty_chunk = empty_chunk_;
    pinned = batch_is_pinned(utf8, offsets, n);
    return KGPU_OK;
}
int ChunkSource::stage(kgpu_ctx *c, uint64_t lo, uint64_t m, const uint8_t *&d_utf8, const uint64_t *&d_offsets) const {
    if (split.c) {   // the input is where the split left it
        d_utf8 = (const uint8_t *)split.c->split_text.p; d_offsets = (const uint64_t *)split.c->split_off.p + lo;
        return KGPU_OK;
    }
    const uint64_t *off = offsets + lo;
    ChunkInput in;
    int rc;
    if ((rc = in.prepare(c, m, off[m] - off[0], !pinned)) || (rc = upload_input(c, in, utf8, off, pinned))) return rc;
    d_utf8 = in.d_text(c, off[0]); d_offsets = in.d_offsets(c);
    return KGPU_OK;
}

// kgpu_tokenize_*_lines, kgpu_tokenize_*_words and kgpu_encode_*: the chunks differ in their renderer alone, the calls in their source.
// (every call takes the chunk pipeline: the single-launch small-call path renders nothing)
static int lines_call(const ChunkSource &src, const Renderer &r, const char *who, LinesSink &sink, uint64_t *n_units) {
    sink.unit = r.unit();
    if (!sink.overflow) sink.text_offsets[0] = 0;
    LinesChunk proto;
    proto.renderer = r;
    const int rc = run_chunks(src, proto, who, [&](ChunkJob<LinesChunk> &j) { return j.out.finish(j.c, j.lo, sink, who); });
    if (n_units) *n_units = sink.text_done;
    return rc;
}

int kgpu::batch_lines(kgpu_dict *d, const Renderer &r, const char *who, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                       uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    if (!d || !offsets || !text_offsets || (text_capacity && !text)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    ChunkSource src;
    int rc;
    if ((rc = src.packed(d, who, utf8, offsets, n, true, true))) return rc;
    LinesSink sink{text, text_capacity, text_offsets, status, true};   // (status has n entries whatever the text buffer holds)
    if ((rc = lines_call(src, r, who, sink, n_bytes)) || !sink.overflow) return rc;
    set_error("%s buffer too small: need %llu, capacity %llu", r.noun(), (unsigned long long)sink.text_done, (unsigned long long)text_capacity);
    return KGPU_ERR_CAPACITY;
}

// The text column (kgpu_tokenize_text_lines / _words, kgpu_encode_text): the chunks' inputs are pointers into the split's output -- nothing of the text
// returns to the host in between.
int kgpu::text_lines(kgpu_dict *d, const Renderer &r, const char *WHO, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                      uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes) {
    if (!d || (len && !text) || (text_capacity && !out_text) || (offsets_capacity && !text_offsets) || !n_lines || !n_bytes) { set_error("%s: null argument", WHO); return KGPU_ERR_INVALID_ARG; }
    *n_lines = 0; *n_bytes = 0;
    ChunkSource src;
    int rc;
    if ((rc = src.block(d, WHO, text, len, true))) return rc;
    *n_lines = src.n;
    LinesSink sink{out_text, text_capacity, text_offsets, status, false};   // (status is bounded by offsets_capacity: nothing of it after an overflow)
    sink.overflow = src.n + 1 > offsets_capacity;
    if ((rc = lines_call(src, r, WHO, sink, n_bytes)) || !sink.overflow) return rc;
    set_error("%s: buffers too small: need %llu text bytes (capacity %llu) and %llu offsets (capacity %llu)", WHO, (unsigned long long)sink.text_done,
              (unsigned long long)text_capacity, (unsigned long long)(src.n + 1), (unsigned long long)offsets_capacity);
    return KGPU_ERR_CAPACITY;
}

extern "C" int kgpu_tokenize_batch_lines(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                         uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    return batch_lines(d, Renderer(), "kgpu_tokenize_batch_lines", utf8, offsets, n, text, text_capacity, text_offsets, status, n_bytes);
}

extern "C" int kgpu_tokenize_batch_words(kgpu_words *w, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                         uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    if (!w) { set_error("kgpu_tokenize_batch_words: null argument"); return KGPU_ERR_INVALID_ARG; }
    return batch_lines(w->dict, Renderer(w), "kgpu_tokenize_batch_words", utf8, offsets, n, text, text_capacity, text_offsets, status, n_bytes);
}

// Pinned, device-visible host memory for the buffers of kgpu_tokenize_batch: the copies then run as DMA
// at PCIe speed and overlap the kernels (pageable memory is staged by the runtime, synchronously).
extern "C" void *kgpu_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, (size_t)(bytes ? bytes : 1), hipHostMallocDefault) != hipSuccess) { set_error("kgpu_host_alloc: %llu bytes failed", (unsigned long long)bytes); return nullptr; }
    return p;
}
extern "C" void kgpu_host_free(void *p) { if (p) (void)hipHostFree(p); }
