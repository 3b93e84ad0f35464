// kanpyo_amd/csrc/kgpu_ctx.cpp -- the contexts of include/kanpyo_gpu.h and the launch chain behind them.
//
// Owns: context create / destroy, the lease of a dictionary's pooled contexts (pool_get / pool_put; the scope guard over them is PooledCtx, kgpu_runtime.h), the stream of a batch (ctx_begin_batch chooses the shared stream by load before the
// batch's first command, ctx_pick_stream places the batch), the one way a batch's host-to-device copy is queued (ctx_h2d), running a batch's chain (kgpu_chain.cpp decides it) with the scan and
// compaction behind it, the reruns in kgpu_ctx_sync, the profiling / ablation / plan getters, the two words a launch publishes to the
// host (HostReport), the render of a batch's lines, and the lattice dump.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "kgpu_runtime.h"

// ----------------------------------------------------------------------- ctx

extern "C" int kgpu_ctx_create(kgpu_dict *d, void *hip_stream, kgpu_ctx **out) {
    if (!d || !out) { set_error("kgpu_ctx_create: null argument"); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    HIPCHECK(hipSetDevice(d->device));
    kgpu_ctx *c = new kgpu_ctx();
    c->dict = d;
    d->refs.fetch_add(1, std::memory_order_relaxed);
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = true; }
    else {
        std::lock_guard<std::mutex> g(d->pool_mu);
        // Streams that really run side by side: HIP gives a process GPU_MAX_HW_QUEUES hardware queues (default 4), of
        // which its streams get one fewer; a stream beyond that shares a queue and unbalances them (4 streams on the
        // default: 52 M sentences/s instead of 68).  Four concurrent launches are the optimum (71.5; five: 58), so:
        // 4 streams when the process was started with GPU_MAX_HW_QUEUES >= 5, else 3.  KGPU_STREAMS overrides.
        // The dictionary's first such context creates them all: a context is not tied to one of them -- each of its batches goes to the least-loaded
        // (ctx_begin_batch), so a single context uses them in turn, and eight contexts load three streams 8 : 8 : 8 over any 24 batches, not 3 : 3 : 2.
        const unsigned n_streams = planned_streams();
        if (!d->stream_load) {
            d->stream_load.reset(new std::atomic<uint64_t>[n_streams]);
            d->stream_batches.reset(new std::atomic<uint64_t>[n_streams]);
            for (unsigned k = 0; k < n_streams; ++k) { d->stream_load[k].store(0, std::memory_order_relaxed); d->stream_batches[k].store(0, std::memory_order_relaxed); }
            d->streams.reserve(n_streams);   // (read without the lock once a context exists: never reallocated)
        }
        while (d->streams.size() < n_streams) {
            hipStream_t st = nullptr;
            hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) { set_error("hipStreamCreate: %s", hipGetErrorString(e)); kgpu_ctx_destroy(c); return KGPU_ERR_HIP; }
            d->streams.push_back(st);
        }
        c->short_idx = pick_stream(d->stream_load.get(), n_streams, d->stream_cursor);   // (until its first batch: what the small calls and the dumps run on)
        c->stream = c->short_stream = d->streams[c->short_idx];
    }
    if (hipMalloc((void **)&c->d_ctl, sizeof(Control)) != hipSuccess ||
        hipHostMalloc((void **)&c->h_ctl, sizeof(Control), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->h_ctl_dev, c->h_ctl, 0) != hipSuccess) {
        set_error("kgpu_ctx_create: control block allocation failed");
        kgpu_ctx_destroy(c);
        return KGPU_ERR_HIP;
    }
    if (hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->switch_ev, hipEventDisableTiming) != hipSuccess) {
        set_error("kgpu_ctx_create: hipEventCreate failed");
        kgpu_ctx_destroy(c);
        return KGPU_ERR_HIP;
    }
    hipDeviceProp_t p;
    const int cus = hipGetDeviceProperties(&p, d->device) == hipSuccess ? p.multiProcessorCount : 256;
    c->plan = make_launch_plan(cus, Occupancy{pool_workgroups_per_cu, window_workgroups_per_cu, window_team_workgroups_per_cu});
    const TestHooks hooks = test_hooks();
    c->aux_mode = hooks.aux_launch;
    c->arena_initial = hooks.arena_initial ? (size_t)std::min<uint64_t>(ARENA_INITIAL, std::max<uint64_t>(1ull << 20, hooks.arena_initial)) : ARENA_INITIAL;
    *out = c;
    return KGPU_OK;
}

// The pending batch is over (completed or given up): the context is free, its share of the dictionary's long sentences in flight and its weight on
// its shared stream are returned.
static void ctx_retire(kgpu_ctx *c) {
    c->pending = false;
    if (c->load_weight) { c->dict->stream_load[c->load_idx].fetch_sub(c->load_weight, std::memory_order_relaxed); c->load_weight = 0; }
    if (c->steer.counted_long) { c->dict->steer.long_sentences_in_flight.fetch_sub(c->steer.counted_long, std::memory_order_relaxed); c->steer.counted_long = 0; }
}

extern "C" void kgpu_ctx_destroy(kgpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->dict->device);
    if (c->pending && c->done_ev) (void)hipEventSynchronize(c->done_ev);
    ctx_retire(c);
    if (c->done_ev) (void)hipEventDestroy(c->done_ev);
    c->lines_report.release(); c->split_report.release();
    c->lines_len.release(); c->lines_text.release(); c->lines_off.release(); c->lines_status.release();
    c->split_agg.release(); c->split_raw.release(); c->split_text.release(); c->split_off.release();
    c->lat_desc.release(); c->lat_words.release(); c->lat_out.release(); c->norm_text.release();
    c->norm_edits.release(); c->norm_eoff.release(); c->span_out.release();
    if (c->switch_ev) (void)hipEventDestroy(c->switch_ev);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    c->arena.release(); c->ovf.release(); c->stat_slots.release(); c->stage.release(); c->tok_count.release();
    c->in_utf8.release(); c->in_off.release(); c->out_tok.release(); c->out_off.release(); c->out_status.release();
    c->pin_in.release(); c->pin_out.release(); c->in_block.release();
    if (c->d_ctl) (void)hipFree(c->d_ctl);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->sm_host) (void)hipHostFree(c->sm_host);
    kgpu_dict *d = c->dict;
    delete c;
    dict_release(d);
}

static int next_event(kgpu_ctx *c, hipEvent_t *ev) {
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e;
        HIPCHECK(hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    *ev = c->ev_pool[c->ev_used++];
    return KGPU_OK;
}

// The head of a batch, before its first command is queued (ctx_h2d: a host-buffer path's copy; else ctx_pick_stream): its shared stream is the least-loaded of
// the dictionary's (kgpu_chain.h: pick_stream).  Chosen HERE and not behind the copy: a batch that left the stream its copy is on would have to wait for an
// event there, behind the other contexts' whole backlog.  The context moves only when nothing of its own is pending where it is -- the tokenize batch retired,
// no lines / count / encode / normalise / split call waiting for its sync -- so its buffers need no ordering between the streams; otherwise it stays.  A
// context that is on its long stream keeps `stream` (the copy goes there, as before; ctx_pick_stream decides where the batch runs).  The caller's own stream: never.
static void ctx_begin_batch(kgpu_ctx *c) {
    if (c->batch_begun) return;
    c->batch_begun = true;
    if (c->own_stream || c->pending || c->lines_report.pending || c->split_report.pending) return;
    kgpu_dict *d = c->dict;
    const bool on_short = c->stream == c->short_stream;
    c->short_idx = pick_stream(d->stream_load.get(), (unsigned)d->streams.size(), d->stream_cursor);
    c->short_stream = d->streams[c->short_idx];
    if (on_short) c->stream = c->short_stream;
}

// The batch is queued on a shared stream: its weight there until ctx_retire (a tail pass or a rerun inside kgpu_ctx_sync stays on the stream and under this weight).
static void ctx_count_load(kgpu_ctx *c, uint64_t total_bytes) {
    if (c->own_stream || c->stream != c->short_stream || c->load_weight) return;
    kgpu_dict *d = c->dict;
    c->load_idx = c->short_idx;
    c->load_weight = stream_batch_weight(total_bytes);
    d->stream_load[c->load_idx].fetch_add(c->load_weight, std::memory_order_relaxed);
    d->stream_batches[c->load_idx].fetch_add(1, std::memory_order_relaxed);
}

// The stream the batch runs on: the short stream ctx_begin_batch chose, or the context's long stream.  A chain that starts with the windowed kernel (kgpu_chain.cpp: starts_with_window) runs on a stream of the long set,
// one per context, so that eight such launches overlap instead of four (cfg 5, 8 in flight: 3.40 -> 3.96 Gchar/s; profiles/experiments/r05_long_chains.txt).
// The context's previous batch is complete here (kgpu_ctx_sync), so switching streams needs no ordering for the context's own buffers; whatever the
// host-buffer paths queued on the old stream for THIS batch (their H2D copy) is ordered in front by an event.
static int ctx_pick_stream(kgpu_ctx *c, const Batch &b) {
    ctx_begin_batch(c);
    c->batch_begun = false;   // (the next ctx_h2d or tokenize call begins the next batch)
    if (c->own_stream) { c->h2d_queued = false; return KGPU_OK; }
    hipStream_t want = c->short_stream;
    // ... and so does a pool-first chain whose last batch sent an eighth or more of its sentences on to the windowed kernel: its launches behind the pool
    // kernel are the long ones (cfg 3 in batches of 4096: 15.4 -> 17.5 M sentences/s on eight streams; a pool-ONLY chain loses there: cfg 2 101 -> 86)
    if ((starts_with_window(c->plan, b) || c->steer.long_share) && planned_long_streams()) {
        if (!c->long_stream) {
            kgpu_dict *d = c->dict;
            std::lock_guard<std::mutex> g(d->pool_mu);
            if (d->long_streams.size() < planned_long_streams()) {
                hipStream_t st = nullptr;
                if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess) d->long_streams.push_back(st);
                else (void)hipGetLastError();
            }
            if (!d->long_streams.empty()) c->long_stream = d->long_streams[d->next_long++ % d->long_streams.size()];
        }
        if (c->long_stream) want = c->long_stream;
    }
    if (want != c->stream) {
        // only what THIS call queued on the old stream (a host-buffer path's H2D copy) has to be in front of the batch; without it no ordering is needed (the
        // context's previous batch is complete) -- and an event on a shared stream would put the batch behind the other contexts' whole backlog there
        if (c->h2d_queued) {
            HIPCHECK(hipEventRecord(c->switch_ev, c->stream));
            HIPCHECK(hipStreamWaitEvent(want, c->switch_ev, 0));
        }
        c->stream = want;
    }
    c->h2d_queued = false;
    return KGPU_OK;
}

// The pending chain (c->chain) on c->stream, then scan + compaction.  ev: timing events {behind the first launch, behind the chain, behind the scan} or null.
static int run_chain(kgpu_ctx *c, const BatchArgs &a, const hipEvent_t *ev, const char *what) {
    const Chain &ch = c->chain;
    if (ev && !ch.event_behind_first) HIPCHECK(hipEventRecord(ev[0], c->stream));
    for (int k = 0; k < ch.n; ++k) {
        hipError_t e = (hipError_t)launch_step(c->dict->view, a, ch.steps[k], c->stop_after, c->stream);
        if (e == hipSuccess && ev && k == 0 && ch.event_behind_first) e = hipEventRecord(ev[0], c->stream);
        if (e != hipSuccess) { set_error("%s launch: %s", what, hipGetErrorString(e)); return KGPU_ERR_HIP; }
    }
    // (the two small kernels behind a pool-only chain on a partner stream of each shared stream, so that the shared stream goes on with the next pool launch at once:
    // measured with 16 hardware queues, cfg 2 100.5 -> 72.9 M sentences/s -- whatever lets a fifth pool launch start early loses, profiles/experiments/r05_long_chains.txt)
    if (ev) HIPCHECK(hipEventRecord(ev[1], c->stream));
    c->h_ctl->pack_overflow = 0;  // set by the compaction's workgroups in the host copy directly; this context's previous batch has been synced
    hipError_t e = (hipError_t)launch_scan_compact(a, c->h_ctl_dev, c->stream, ch.small_scan, ch.aux_one_launch, c->aux_mode, &c->aux_form);
    if (e != hipSuccess) { set_error("scan/compact launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    if (ev) HIPCHECK(hipEventRecord(ev[2], c->stream));
    HIPCHECK(hipEventRecord(c->done_ev, c->stream));
    c->ctl_dirty = false;
    c->pending = true;
    return KGPU_OK;
}

static int enqueue(kgpu_ctx *c, const BatchArgs &a, const Batch &b) {
    // The Control block is zero here: the previous launch's scan kernel left it so.
    if (c->ctl_dirty) HIPCHECK(hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream));
    c->ctl_dirty = true;  // until this enqueue is through
    hipEvent_t ev[4] = {};
    int rc;
    const bool timed = c->profiling && (c->launch_seq++ % c->event_every) == 0;
    if (timed) {
        for (hipEvent_t &e : ev) if ((rc = next_event(c, &e))) return rc;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
    }
    c->chain = build_chain(c->plan, b, c->dict->steer, c->steer);
    c->last = a;
    return run_chain(c, a, timed ? ev + 1 : nullptr, "k_tokenize");
}

static int tokenize_batch(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                          kgpu_token *d_tokens, kgpu_token8 *d_tokens8, uint32_t *d_first, uint8_t *status8, uint64_t *toff8, uint64_t token_capacity,
                          uint64_t *d_tok_offsets, uint8_t *d_status, const char *who);

// A batch on the context: tokenize_batch below.  However it fails, the context is left without a batch begun -- the next batch chooses its stream anew -- and,
// if a host-buffer path had queued this batch's copy, with that copy through: it writes the context's input block, which the next batch's copy on
// another stream writes again (an error path: the wait behind a shared stream's backlog costs nothing that matters).
int kgpu::tokenize_device_impl(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                                kgpu_token *d_tokens, kgpu_token8 *d_tokens8, uint32_t *d_first, uint8_t *status8, uint64_t *toff8, uint64_t token_capacity,
                                uint64_t *d_tok_offsets, uint8_t *d_status, const char *who) {
    const int rc = tokenize_batch(c, d_utf8, d_offsets, n, total_bytes, d_tokens, d_tokens8, d_first, status8, toff8, token_capacity, d_tok_offsets, d_status, who);
    if (rc && c) {
        if (c->h2d_queued && !c->pending) (void)hipStreamSynchronize(c->stream);
        c->batch_begun = c->h2d_queued = false;
    }
    return rc;
}

static int tokenize_batch(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                          kgpu_token *d_tokens, kgpu_token8 *d_tokens8, uint32_t *d_first, uint8_t *status8, uint64_t *toff8, uint64_t token_capacity,
                          uint64_t *d_tok_offsets, uint8_t *d_status, const char *who) {
    if (!c || !d_offsets || !d_tok_offsets || (n && !d_status) || (total_bytes && !d_utf8) ||
        (token_capacity && !d_tokens && !d_tokens8) || (d_tokens8 && n && !d_first)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (n >= (1ull << 32) - 1) { set_error("%s: more than 2^32-2 sentences in one batch; split it", who); return KGPU_ERR_INVALID_ARG; }
    if (total_bytes >= (1ull << 32)) { set_error("%s: batch larger than 4 GiB; split it", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    int rc;
    if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    const Batch b{n, total_bytes, c->dict->steer.est_q8.load(std::memory_order_relaxed), c->stop_after, false, false, c->rt.batches > 0};
    if ((rc = ctx_pick_stream(c, b))) return rc;
    if ((rc = c->arena.ensure(c->arena_initial)) || (rc = c->stage.ensure((size_t)token_bound(total_bytes, n) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure((size_t)(n + 1) * 4)) ||
        (rc = c->ovf.ensure((size_t)(n + 1) * 4 * 4)))
        return rc;
    BatchArgs a{};
    a.utf8 = d_utf8; a.offsets = d_offsets; a.n = n; a.ctl = c->d_ctl;
    a.arena = (uint8_t *)c->arena.p; a.arena_bytes = c->arena.bytes;
    a.stage = (kgpu_token *)c->stage.p;
    a.tok_count = (uint32_t *)c->tok_count.p;
    a.status = d_status; a.out = d_tokens; a.out_cap = token_capacity; a.tok_offsets = d_tok_offsets;
    a.out8 = d_tokens8; a.first8 = d_first; a.status8 = status8; a.toff8 = toff8;
    a.count_work = c->count_work ? (c->count_no_t ? 3u : 1u) : 0u;
#ifdef KGPU_STEP_TIMING
    const bool want_stats = true;
#else
    const bool want_stats = c->count_work;
#endif
    if (want_stats) {
        if (!c->stat_slots.p) {
            if ((rc = c->stat_slots.ensure((size_t)STAT_SLOTS * STAT_WORDS * 8))) return rc;
            HIPCHECK(hipMemsetAsync(c->stat_slots.p, 0, (size_t)STAT_SLOTS * STAT_WORDS * 8, c->stream));
        }
        a.stat_slots = (unsigned long long *)c->stat_slots.p;
    }
    a.est_q8 = b.est_q8;
    for (int k = 0; k < 4; ++k) a.ovf[k] = (uint32_t *)c->ovf.p + (size_t)k * (n + 1);
    c->batch = b;
    if ((rc = enqueue(c, a, b))) return rc;
    ctx_count_load(c, total_bytes);
    return KGPU_OK;
}

// The tail chain (c->chain) over work list `li` of the pending batch, which the first chain left unserved, then scan + compaction again.
static int enqueue_tail(kgpu_ctx *c, int li) {
    // (the scan kernel zeroed the control block after publishing it; the completed batch is behind us on the stream)
    HIPCHECK(hipMemcpyAsync(&c->d_ctl->ovf_count[li], &c->tail_saved.ovf_count[li], sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    c->ctl_dirty = true;
    return run_chain(c, c->last, nullptr, "tail");
}

extern "C" int kgpu_tokenize_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                    uint64_t total_bytes, kgpu_token *d_tokens, uint64_t token_capacity,
                                    uint64_t *d_tok_offsets, uint8_t *d_status) {
    return tokenize_device_impl(c, d_utf8, d_offsets, n, total_bytes, d_tokens, nullptr, nullptr, nullptr, nullptr, token_capacity, d_tok_offsets, d_status,
                                "kgpu_tokenize_device");
}

extern "C" int kgpu_tokenize_device_compact(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                            uint64_t total_bytes, kgpu_token8 *d_tokens8, uint64_t token_capacity,
                                            uint32_t *d_first, uint64_t *d_tok_offsets, uint8_t *d_status) {
    if (token_capacity && !d_tokens8) { set_error("kgpu_tokenize_device_compact: null argument"); return KGPU_ERR_INVALID_ARG; }
    return tokenize_device_impl(c, d_utf8, d_offsets, n, total_bytes, nullptr, d_tokens8, d_first, nullptr, nullptr, token_capacity, d_tok_offsets, d_status,
                                "kgpu_tokenize_device_compact");
}

// Host side of the 8-byte records: position / start are running sums over the sentence (include/kanpyo_gpu.h, kgpu_token8).
extern "C" void kgpu_expand_tokens(const kgpu_token8 *in, const uint64_t *tok_offsets, const uint32_t *first, uint64_t n, kgpu_token *out) {
    const bool stream = n && expand_stream_wanted(tok_offsets[n] - tok_offsets[0]);
    expand_tokens(in, tok_offsets, first, n, out, stream);
    if (stream) expand_fence();
}

extern "C" int kgpu_ctx_sync(kgpu_ctx *c, uint64_t *n_tokens) {
    if (!c) { set_error("kgpu_ctx_sync: null ctx"); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    for (;;) {
        if (!c->pending) { if (n_tokens) *n_tokens = 0; return KGPU_OK; }
        HIPCHECK(hipEventSynchronize(c->done_ev));  // this context's batch only: later work on a shared stream is not waited for
        if (c->h_ctl->window_fail && !c->h_ctl->arena_overflow) {
            // the windowed kernel met a sentence it cannot hold and had no list to hand it on to: the batch once more without it
            c->rt.window_reruns++;
            // the rerun counts everything again: drop what this run left in the per-wavefront slots
            if (c->last.stat_slots) HIPCHECK(hipMemsetAsync(c->last.stat_slots, 0, (size_t)STAT_SLOTS * STAT_WORDS * 8, c->stream));
            c->tail_pass = false;
            Batch b = c->batch;
            b.no_window = true;
            int rc = enqueue(c, c->last, b);
            if (rc) { ctx_retire(c); return rc; }
            continue;
        }
        const int li = c->chain.last_list();
        if (li >= 0 && !c->h_ctl->arena_overflow && c->h_ctl->ovf_count[li] > 0) {
            // The chain ended without its tail and a sentence needed it: ONLY what is missing (the windowed kernel if it was not in the chain,
            // then the general kernel), over the last work list (still in device memory; its length goes back into the control block the scan
            // kernel zeroed), then scan + compaction once more.  The pool kernel's work is not repeated: a corpus with a sparse but steady
            // share of long sentences pays a small launch per such batch, not the batch twice.  What the first pass counted (routing,
            // estimate feedback, work counters) is kept and merged below.
            c->rt.tail_reruns++;
            c->tail_saved = *c->h_ctl;
            c->tail_pass = true;
            c->first_pass = c->chain;
            c->chain = tail_chain(c->plan, c->first_pass);
            int rc = enqueue_tail(c, li);
            if (rc) { ctx_retire(c); c->tail_pass = false; return rc; }
            continue;
        }
        if (c->h_ctl->arena_overflow) {
            // a lattice did not fit the scratch arena: grow it and redo the batch
            size_t want = c->arena.bytes * 2;
            if (want > ARENA_MAX) { set_error("scratch arena exceeded %zu bytes", ARENA_MAX); ctx_retire(c); return KGPU_ERR_INTERNAL; }
            int rc = c->arena.ensure(want);
            if (rc) { ctx_retire(c); return rc; }
            BatchArgs a = c->last;
            a.arena = (uint8_t *)c->arena.p; a.arena_bytes = c->arena.bytes;
            c->rt.arena_regrows++;
            // (the windowed kernel counted the sentences it flagged for want of a chunk under whys 3 and 5: kept, the run's control block goes with the rerun;
            // what the run handed on for other reasons is handed on again, and counted, by the run that stands)
            if (!c->last.count_work) for (int k = 3; k <= 5; k += 2) c->rt.window_handed[k] += c->h_ctl->phase[k] + (c->tail_pass ? c->tail_saved.phase[k] : 0);
            c->tail_pass = false;  // (the whole batch runs again: nothing of an earlier pass is merged)
            // the rerun counts everything again: drop what the aborted run left in the per-wavefront slots (ctl->work went with the control block)
            if (a.stat_slots) HIPCHECK(hipMemsetAsync(a.stat_slots, 0, (size_t)STAT_SLOTS * STAT_WORDS * 8, c->stream));
            if ((rc = enqueue(c, a, c->batch))) { ctx_retire(c); return rc; }
            continue;
        }
        break;
    }
    ctx_retire(c);
    const Chain &first = c->tail_pass ? c->first_pass : c->chain;   // what the FIRST pass of this batch had in its chain (the arming decays on that)
    const Chain *tail = c->tail_pass ? &c->chain : nullptr;
    if (c->tail_pass) {   // the published block is the tail pass's: put back what the first pass had counted
        c->tail_pass = false;
        Control &h = *c->h_ctl;
        const Control &sv = c->tail_saved;
        for (int k = 0; k < 4; ++k) { if (k <= first.last_list()) h.ovf_count[k] = sv.ovf_count[k]; h.late_count[k] += sv.late_count[k]; }   // lists up to the one the tail served are the first pass's
        for (int k = 0; k < 7; ++k) h.work[k] += sv.work[k];
        for (int k = 0; k < 10; ++k) h.phase[k] += sv.phase[k];
        h.pack_overflow |= sv.pack_overflow;
    }
    c->rt.batches++; c->rt.sentences += c->last.n;
    for (int k = 0; k < 4; ++k) { c->rt.deferred[k] += c->h_ctl->ovf_count[k]; c->rt.redone[k] += c->h_ctl->late_count[k]; }
    if (first.find(Kernel::Window) || (tail && tail->find(Kernel::Window))) c->rt.long_launches++;
    chain_feedback(c->plan, first, tail, *c->h_ctl, c->last.n, c->last.est_q8, c->dict->steer, c->steer);
    if (c->profiling) {
        for (size_t i = 0; i + 4 <= c->ev_used; i += 4) {
            float t0f = 0, t01 = 0, t12 = 0;
            if (hipEventElapsedTime(&t0f, c->ev_pool[i], c->ev_pool[i + 1]) == hipSuccess &&
                hipEventElapsedTime(&t01, c->ev_pool[i], c->ev_pool[i + 2]) == hipSuccess &&
                hipEventElapsedTime(&t12, c->ev_pool[i + 2], c->ev_pool[i + 3]) == hipSuccess) {
                c->prof.launches++; c->rt.first_ms += t0f; c->prof.tokenize_ms += t01; c->prof.aux_ms += t12;
            }
        }
        c->ev_used = 0;
    }
    if (!c->last.count_work) for (int k = 0; k < 10; ++k) c->rt.window_handed[k] += c->h_ctl->phase[k];   // (Control::phase: the windowed kernel's reasons, when it holds no clocks)
    if (c->last.count_work) {  // what the general kernels counted (atomics on the control block)
        const unsigned long long *w = c->h_ctl->work;
        c->work.sentences += w[0]; c->work.B += w[1]; c->work.C += w[2]; c->work.T += w[3];
        c->work.N += w[4]; c->work.E += w[5]; c->work.K += w[6];
        for (int k = 0; k < 10; ++k) c->phase[k] += c->h_ctl->phase[k];
    }
    if (c->last.stat_slots) {  // ... and the pool kernel's wavefronts, each in its own slot
        const size_t words = (size_t)STAT_SLOTS * STAT_WORDS;
        c->stat_host.resize(words);
        HIPCHECK(hipMemcpyAsync(c->stat_host.data(), c->last.stat_slots, words * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemsetAsync(c->last.stat_slots, 0, words * 8, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        unsigned long long sum[STAT_WORDS] = {0};
        for (size_t i = 0; i < words; ++i) sum[i % STAT_WORDS] += c->stat_host[i];
        c->work.sentences += sum[0]; c->work.B += sum[1]; c->work.C += sum[2]; c->work.T += sum[3];
        c->work.N += sum[4]; c->work.E += sum[5]; c->work.K += sum[6];
        for (int k = 0; k < 10; ++k) c->phase[k] += sum[16 + k];
    }
    uint64_t need = c->h_ctl->n_tokens;
    if (c->last.out8 && c->h_ctl->pack_overflow) {
        if (n_tokens) *n_tokens = 0;
        set_error("a token does not fit the 8-byte record (more than 4095 chars or 262143 bytes): use the 24-byte form for this batch");
        return KGPU_ERR_CAPACITY;
    }
    if (n_tokens) *n_tokens = need;
    if (c->h_ctl->n_tokens > c->last.out_cap) {
        set_error("token buffer too small: need %llu, capacity %llu", (unsigned long long)need, (unsigned long long)c->last.out_cap);
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}

// Tests only (not in the header): the form of the context's last scan + compaction, as launch_scan_compact numbers it (0: none yet).
extern "C" int kgpu_debug_aux_form(kgpu_ctx *c) { return c ? c->aux_form : -1; }
// ... and how many batches each of the dictionary's shared streams has been given since the last reset: -> the number of shared streams (0: none created yet),
// the first `cap` of their counts in out[].
extern "C" int kgpu_debug_stream_batches(kgpu_dict *d, uint64_t *out, int cap, int reset) {
    if (!d) return -1;
    std::lock_guard<std::mutex> g(d->pool_mu);
    const int n = (int)d->streams.size();
    if (!d->stream_batches || n < (int)planned_streams()) return 0;
    for (int k = 0; k < n; ++k) {
        const uint64_t v = reset ? d->stream_batches[k].exchange(0, std::memory_order_relaxed) : d->stream_batches[k].load(std::memory_order_relaxed);
        if (out && k < cap) out[k] = v;
    }
    return n;
}

extern "C" int kgpu_ctx_set_profiling(kgpu_ctx *c, int mode) {
    if (!c) { set_error("kgpu_ctx_set_profiling: null ctx"); return KGPU_ERR_INVALID_ARG; }
    c->profiling = (mode & KGPU_PROFILE_EVENTS) != 0;
    c->event_every = (mode & KGPU_PROFILE_SAMPLED) ? 4u : 1u;
    c->launch_seq = 0;
    c->count_work = (mode & KGPU_PROFILE_WORK) != 0;
    c->count_no_t = (mode & KGPU_PROFILE_NO_T) != 0;
    return KGPU_OK;
}

extern "C" int kgpu_ctx_set_ablation(kgpu_ctx *c, int stop_after_stage) {
    if (!c || stop_after_stage < 0 || stop_after_stage > 7) { set_error("kgpu_ctx_set_ablation: bad argument"); return KGPU_ERR_INVALID_ARG; }
    c->stop_after = (uint32_t)stop_after_stage;
    return KGPU_OK;
}

extern "C" int kgpu_ctx_get_phase_cycles(kgpu_ctx *c, uint64_t out[10], int reset) {
    if (!c || !out) { set_error("kgpu_ctx_get_phase_cycles: null argument"); return KGPU_ERR_INVALID_ARG; }
    for (int k = 0; k < 10; ++k) { out[k] = c->phase[k]; if (reset) c->phase[k] = 0; }
    return KGPU_OK;
}

extern "C" int kgpu_ctx_get_work(kgpu_ctx *c, kgpu_work *out, int reset) {
    if (!c || !out) { set_error("kgpu_ctx_get_work: null argument"); return KGPU_ERR_INVALID_ARG; }
    *out = c->work;
    if (reset) c->work = kgpu_work{};
    return KGPU_OK;
}

extern "C" int kgpu_ctx_get_profile(kgpu_ctx *c, kgpu_profile *out, int reset) {
    if (!c || !out) { set_error("kgpu_ctx_get_profile: null argument"); return KGPU_ERR_INVALID_ARG; }
    *out = c->prof;
    if (reset) c->prof = kgpu_profile{};
    return KGPU_OK;
}

extern "C" int kgpu_ctx_get_plan(kgpu_ctx *c, kgpu_plan_info *out, size_t out_size) {
    if (!c || !out || out_size < 4) { set_error("kgpu_ctx_get_plan: bad argument"); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    kgpu_plan_info p{};
    hipDeviceProp_t prop;
    p.compute_units = hipGetDeviceProperties(&prop, c->dict->device) == hipSuccess ? (uint32_t)prop.multiProcessorCount : 0u;
    if (c->plan.n_pools) {
        p.pool_lds_bytes = c->plan.pool_bytes[0]; p.pool_wavefronts = c->plan.pool_waves[0]; p.pool_max_pages = c->plan.pool_max_pages[0];
        p.pool_workgroups_per_cu = (uint32_t)pool_workgroups_per_cu(c->plan.pool_bytes[0], c->plan.pool_waves[0]);
    }
    p.window_lds_bytes = c->plan.window_lds_bytes; p.window_workgroups = (uint32_t)c->plan.window_workgroups;
    p.window_workgroups_per_cu = c->plan.window_lds_bytes ? (uint32_t)window_workgroups_per_cu(c->plan.window_lds_bytes) : 0u;
    p.streams = planned_streams();
    p.long_streams = c->own_stream ? 0u : planned_long_streams();
    p.window_first_bytes = (c->plan.n_pools && c->plan.window_lds_bytes) ? c->plan.window_first_bytes : 0u;
    std::memcpy(out, &p, std::min(out_size, sizeof p));
    return KGPU_OK;
}

extern "C" int kgpu_ctx_get_routing(kgpu_ctx *c, kgpu_routing *out, size_t out_size, int reset) {
    if (!c || !out || out_size < 8) { set_error("kgpu_ctx_get_routing: bad argument"); return KGPU_ERR_INVALID_ARG; }
    std::memcpy(out, &c->rt, std::min(out_size, sizeof(kgpu_routing)));
    if (reset) c->rt = kgpu_routing{};
    return KGPU_OK;
}

// ------------------------------------------------------- a launch's two words for the host (kgpu_runtime.h: HostReport)
int HostReport::arm() {
    if (pending) { pending = false; HIPCHECK(hipEventSynchronize(ev)); }
    if (int rc = ctl.ensure(16, true)) return rc;
    if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    unsigned long long *h = (unsigned long long *)ctl.h;
    h[0] = 0; h[1] = 0;
    two_sizes = false; cap1 = 0; word1 = 0; bad_what = nullptr;
    return KGPU_OK;
}
int HostReport::record(hipStream_t stream, uint64_t cap_) {
    HIPCHECK(hipEventRecord(ev, stream));
    pending = true;
    cap = cap_;
    return KGPU_OK;
}
int HostReport::wait(uint64_t words[2]) {
    pending = false;
    HIPCHECK(hipEventSynchronize(ev));
    const unsigned long long *h = (const unsigned long long *)ctl.h;
    words[0] = h[0]; words[1] = h[1];
    return KGPU_OK;
}
void HostReport::release() {
    if (pending && ev) (void)hipEventSynchronize(ev);
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr; pending = false;
    ctl.release();
}

// ------------------------------------------------------- the CLI's output lines (kgpu_format.hip; reference src/bin/kanpyo.rs:174-197)
int kgpu::require_features(kgpu_dict *d, const char *who) {
    std::lock_guard<std::mutex> g(d->feat_mu);
    if (!d->feat) { set_error("%s: the dictionary has no feature tables: call kgpu_dict_set_features first", who); return KGPU_ERR_INVALID_ARG; }
    return KGPU_OK;
}
int kgpu::begin_records_call(kgpu_ctx *c, const char *who) {
    if (c->pending) { set_error("%s: the context's tokenize batch is not synced (kgpu_ctx_sync) yet", who); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    int rc;
    if (c->lines_report.pending && (rc = kgpu_ctx_sync_lines(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    return KGPU_OK;
}
int kgpu::records_batch(kgpu_ctx *c, const DeviceRecords &r, size_t scratch_bytes, uint64_t *d_unit_offsets, RecordsBatch &b) {
    int rc;
    if ((rc = c->lines_report.arm()) || (rc = c->lines_len.ensure(scratch_bytes))) return rc;
    const kgpu_dict_info &di = c->dict->info;
    b = RecordsBatch{r.d_utf8, r.d_offsets, r.n, r.d_tokens, r.d_tok_offsets, (uint32_t)di.n_morphs, (uint32_t)(di.n_morphs + di.n_unk_morphs),
                     (uint64_t *)c->lines_len.p, d_unit_offsets, r.status_in, r.status_out, c->lines_report.dev()};
    return KGPU_OK;
}
int kgpu::records_launched(kgpu_ctx *c, int launch_error, const char *who, const char *what, uint64_t capacity) {
    if (launch_error != (int)hipSuccess) { set_error("%s: %s launch: %s", who, what, hipGetErrorString((hipError_t)launch_error)); return KGPU_ERR_HIP; }
    return c->lines_report.record(c->stream, capacity);
}
int kgpu::enqueue_lines(kgpu_ctx *c, const DeviceRecords &r, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, const char *who) {
    kgpu_dict *d = c->dict;
    LinesArgs a{};
    int rc;
    if ((rc = require_features(d, who)) || (rc = records_batch(c, r, (size_t)r.n * 8 + 8, d_text_offsets, a.b))) return rc;
    a.feat = d->feat; a.feat_off = d->feat_off;
    a.text = d_text; a.text_cap = text_capacity;
    return records_launched(c, launch_format_lines(a, c->stream), who, "render", text_capacity);
}

extern "C" int kgpu_format_lines_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                        const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                                        uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets) {
    const char *who = "kgpu_format_lines_device";
    if (!c || !d_offsets || !d_tok_offsets || !d_text_offsets || (n && (!d_utf8 || !d_tokens)) || (text_capacity && !d_text)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_lines(c, DeviceRecords{d_utf8, d_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, d_text, text_capacity, d_text_offsets, who);
}

extern "C" int kgpu_ctx_sync_lines(kgpu_ctx *c, uint64_t *n_bytes) {
    if (!c) { set_error("kgpu_ctx_sync_lines: null ctx"); return KGPU_ERR_INVALID_ARG; }
    if (!c->lines_report.pending) { if (n_bytes) *n_bytes = 0; return KGPU_OK; }
    HIPCHECK(hipSetDevice(c->dict->device));
    uint64_t h[2];   // [0] bytes, [1] a bad record -- or, behind an aligned normalise, its edits
    if (int rc = c->lines_report.wait(h)) return rc;
    const uint64_t need = h[0];
    if (n_bytes) *n_bytes = need;
    if (c->lines_report.two_sizes) {
        c->lines_report.word1 = h[1];
        if (need > c->lines_report.cap || h[1] > c->lines_report.cap1) {
            set_error("buffers too small: need %llu text bytes (capacity %llu) and %llu edit records (capacity %llu)", (unsigned long long)need,
                      (unsigned long long)c->lines_report.cap, (unsigned long long)h[1], (unsigned long long)c->lines_report.cap1);
            return KGPU_ERR_CAPACITY;
        }
        return KGPU_OK;
    }
    if (h[1]) {
        if (c->lines_report.bad_what) set_error("kgpu_ctx_sync_lines: %s", c->lines_report.bad_what);
        else set_error("kgpu_ctx_sync_lines: a token record names a class, morph id or surface outside the dictionary or its sentence");
        return KGPU_ERR_INVALID_ARG;
    }
    if (need > c->lines_report.cap) {
        set_error("text buffer too small: need %llu, capacity %llu", (unsigned long long)need, (unsigned long long)c->lines_report.cap);
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}

// ------------------------------------------------------- the lease of pooled contexts, the H2D copy in front of a batch
// the pooled contexts of a dictionary (one per call in flight): every path that borrows a context takes it here and gives it back here
int kgpu::pool_get(kgpu_dict *d, kgpu_ctx **out) {
    kgpu_ctx *c = nullptr;
    {
        std::lock_guard<std::mutex> g(d->pool_mu);
        if (!d->pool.empty()) { c = d->pool.back(); d->pool.pop_back(); }
    }
    if (!c) { int rc = kgpu_ctx_create(d, nullptr, &c); if (rc) return rc; }
    *out = c;
    return KGPU_OK;
}
void kgpu::pool_put(kgpu_dict *d, kgpu_ctx *c) {
    c->batch_begun = c->h2d_queued = false;   // (a path that waited for its ctx_h2d copies itself, without a tokenize batch behind them)
    std::lock_guard<std::mutex> g(d->pool_mu);
    d->pool.push_back(c);
}

// A host-buffer path's copy of a batch's input, queued in front of the batch on the stream ctx_begin_batch chooses for it: the flag makes ctx_pick_stream
// order the batch behind the copy if the batch goes to another stream (a long one).  Everything a path queues ahead of tokenize_device_impl goes through here.
int kgpu::ctx_h2d(kgpu_ctx *c, void *dst, const void *src, size_t bytes, const char *what) {
    ctx_begin_batch(c);
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return KGPU_ERR_HIP; }
    c->h2d_queued = true;
    return KGPU_OK;
}

// ----------------------------------------------------------------- lattice dump
extern "C" int kgpu_lattice_dump(kgpu_dict *d, const uint8_t *utf8, uint64_t len, kgpu_lattice *out) {
    if (!d || !out || (len && !utf8)) { set_error("kgpu_lattice_dump: null argument"); return KGPU_ERR_INVALID_ARG; }
    if (len >= (1ull << 31)) { set_error("kgpu_lattice_dump: sentence too long"); return KGPU_ERR_INVALID_ARG; }
    *out = kgpu_lattice{};
    HIPCHECK(hipSetDevice(d->device));
    PooledCtx lease(d);   // (the copies below go on c->stream, where the dump's own launch follows and is waited for: no batch is begun)
    kgpu_ctx *c = lease.c;
    int rc = lease.rc;
    if (rc) return rc;
    const uint64_t offs[2] = {0, len};
    Control hc{};
    if ((c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) ||
        (rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)(len + 2) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure(8)) || (rc = c->in_utf8.ensure((size_t)len + 16)) || (rc = c->in_off.ensure(16)) ||
        (rc = c->out_status.ensure(16))) return rc;
    auto fail = [&](hipError_t e, const char *what) { set_error("kgpu_lattice_dump: %s: %s", what, hipGetErrorString(e)); c->ctl_dirty = true; return KGPU_ERR_HIP; };
    hipError_t e;
    if (len && (e = hipMemcpyAsync(c->in_utf8.p, utf8, (size_t)len, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "H2D");
    if ((e = hipMemcpyAsync(c->in_off.p, offs, 16, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "H2D");
    for (;;) {
        BatchArgs a{};
        a.utf8 = (const uint8_t *)c->in_utf8.p; a.offsets = (const uint64_t *)c->in_off.p; a.n = 1; a.ctl = c->d_ctl;
        a.arena = (uint8_t *)c->arena.p; a.arena_bytes = c->arena.bytes;
        a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p; a.status = (uint8_t *)c->out_status.p;
        a.dump_lattice = 1;
        c->ctl_dirty = true;  // no scan kernel behind this launch: the next batch zeroes the block itself
        if ((e = hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream)) != hipSuccess) return fail(e, "memset");
        if ((e = (hipError_t)launch_general_only(d->view, a, c->stream)) != hipSuccess) return fail(e, "launch");
        if ((e = hipMemcpyAsync(&hc, c->d_ctl, sizeof(Control), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return fail(e, "D2H");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(e, "sync");
        if (!hc.arena_overflow) break;
        size_t want = c->arena.bytes * 2;
        if (want > ARENA_MAX) { set_error("scratch arena exceeded %zu bytes", ARENA_MAX); return KGPU_ERR_INTERNAL; }
        if ((rc = c->arena.ensure(want))) return rc;
    }
    if (!hc.dump[LAT_VALID]) { set_error("kgpu_lattice_dump: the sentence is not valid UTF-8"); return KGPU_ERR_INVALID_ARG; }
    const uint64_t B = hc.dump[LAT_B], C = hc.dump[LAT_C], N = hc.dump[LAT_N], na = B + 4;
    std::vector<uint32_t> cbyte(C + 1), boff(C + 2), pre(N);
    std::vector<uint32_t> nodeA(4 * N), bucket(4 * N), nodeB(2 * N);
    const uint8_t *sa = (const uint8_t *)c->arena.p + hc.dump[LAT_SLAB_A], *sn = (const uint8_t *)c->arena.p + hc.dump[LAT_SLAB_N];
    // slab layouts: k_tokenize_general (kgpu_kernels.hip): cbyte | uspan | nb | boff | ... (u32[na] each); nodeA | bucket | nodeB | pre
    if ((e = hipMemcpy(cbyte.data(), sa, (C + 1) * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(boff.data(), sa + 3 * na * 4, (C + 2) * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(nodeA.data(), sn, N * 16, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(bucket.data(), sn + N * 16, N * 16, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(nodeB.data(), sn + N * 32, N * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(pre.data(), sn + N * 40, N * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "slab read-back");
    lease.put();   // (the rest is host work)
    out->n_nodes = N; out->n_positions = C + 2;
    out->nodes = (kgpu_lattice_node *)calloc((size_t)N, sizeof(kgpu_lattice_node));
    out->edge_offsets = (uint32_t *)calloc((size_t)C + 3, 4);
    out->edge_nodes = (uint32_t *)calloc((size_t)N, 4);
    if (!out->nodes || !out->edge_offsets || !out->edge_nodes) { kgpu_lattice_free(out); set_error("kgpu_lattice_dump: out of memory"); return KGPU_ERR_INTERNAL; }
    auto orig = [](const std::vector<uint32_t> &inv, uint32_t r) { return (int16_t)(inv.empty() || r >= inv.size() ? r : inv[r]); };
    for (uint64_t t = 0; t < N; ++t) {
        kgpu_lattice_node &nd = out->nodes[t];
        if (t == 0) { nd.pre = -1; continue; }  // BOS: Dummy at 0 with Morph(0, 0, 0); dp None
        const uint32_t *A = &nodeA[4 * t];
        const int32_t sid = (int32_t)A[3];
        const uint32_t st = nodeB[2 * t], en = nodeB[2 * t + 1];
        nd.id = sid < 0 ? -sid : sid;
        nd.cls = sid > 0 ? KGPU_CLASS_KNOWN : sid < 0 ? KGPU_CLASS_UNKNOWN : KGPU_CLASS_DUMMY;
        nd.char_pos = st; nd.end_char = en; nd.byte_pos = cbyte[st]; nd.byte_len = cbyte[en] - cbyte[st];
        if (sid != 0) { nd.left_id = orig(d->left_of_rank, A[0] & 0xFFFFu); nd.right_id = orig(d->right_of_rank, A[0] >> 16); nd.cost = (int16_t)(int32_t)A[1]; }
        nd.dp = A[2] == 0xFFFFFFFFu ? (int32_t)hc.dump[LAT_EOS_DP] : (int32_t)bucket[4 * A[2]];
        nd.pre = pre[t] == 0xFFFFFFFFu ? -1 : (int32_t)pre[t];
    }
    // edges[e] = nodes ending at e, ascending node index (the kernel fills a bucket in arrival order)
    for (uint64_t e2 = 0; e2 <= C + 1; ++e2) out->edge_offsets[e2] = e2 <= C + 1 && e2 < boff.size() ? boff[e2] : 0;
    out->edge_offsets[C + 1] = (uint32_t)(N - 1); out->edge_offsets[C + 2] = (uint32_t)N;
    for (uint64_t sl = 0; sl + 1 < N; ++sl) out->edge_nodes[sl] = bucket[4 * sl + 2];
    out->edge_nodes[N - 1] = (uint32_t)(N - 1);
    for (uint64_t e2 = 0; e2 <= C; ++e2) std::sort(out->edge_nodes + out->edge_offsets[e2], out->edge_nodes + out->edge_offsets[e2 + 1]);
    return KGPU_OK;
}

extern "C" void kgpu_lattice_free(kgpu_lattice *l) {
    if (!l) return;
    free(l->nodes); free(l->edge_offsets); free(l->edge_nodes);
    *l = kgpu_lattice{};
}
