// kanpyo_amd/csrc/kgpu_ctx.cpp -- the contexts of include/kanpyo_gpu.h and the launch chain behind them.
//
// Owns: context create / destroy, the lease of a dictionary's pooled contexts, the choice of chain and stream per batch
// (ctx_pick_chain), the one way a batch's host-to-device copy is queued (ctx_h2d), the launch sequence (tokenize -> scan ->
// compact) and its reruns in kgpu_ctx_sync, the profiling / ablation / plan getters, and the lattice dump.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "kgpu_runtime.h"

// ----------------------------------------------------------------------- ctx

static constexpr size_t ARENA_INITIAL = 1ull << 28;  // 256 MiB; only the general (HBM-scratch) kernel uses it, grows x2 on demand
static constexpr size_t ARENA_MAX = 1ull << 37;      // 128 GiB

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
        const unsigned n_streams = planned_streams();
        if (d->streams.size() < n_streams) {
            hipStream_t st = nullptr;
            hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) { set_error("hipStreamCreate: %s", hipGetErrorString(e)); kgpu_ctx_destroy(c); return KGPU_ERR_HIP; }
            d->streams.push_back(st);
            c->stream = st;
        } else {
            c->stream = d->streams[d->next_stream++ % d->streams.size()];
        }
        c->short_stream = c->stream;
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
    c->plan = default_launch_plan(d->device);
    *out = c;
    return KGPU_OK;
}

extern "C" void kgpu_ctx_destroy(kgpu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->dict->device);
    if (c->pending && c->done_ev) (void)hipEventSynchronize(c->done_ev);
    if (c->counted_long) { c->dict->long_sentences_in_flight.fetch_sub(c->counted_long, std::memory_order_relaxed); c->counted_long = 0; }
    if (c->done_ev) (void)hipEventDestroy(c->done_ev);
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

// Which chain the next batch gets, and on which stream.  A batch of long sentences (by its average length: the host knows n and the bytes, not the
// lengths) starts with the windowed kernel -- the pool launch in front of it would only route: a thousand 40 KB workgroups that each look at four sentences
// and pass them on, waiting for LDS on a chip full of single-wavefront workgroups (cfg 5, 8 in flight: 2.97 -> 3.40 Gchar/s without it) -- and runs on a stream
// of the long set, one per context, so that eight such launches overlap instead of four (-> 3.96; both: profiles/experiments/r05_long_chains.txt).
// The context's previous batch is complete here (kgpu_ctx_sync), so switching streams needs no ordering for the context's own buffers; whatever the
// host-buffer paths queued on the old stream for THIS batch (their H2D copy) is ordered in front by an event.
static int ctx_pick_chain(kgpu_ctx *c, uint64_t n, uint64_t total_bytes, bool dump) {
    const unsigned lim = c->plan.window_first_bytes;   // (KGPU_WINDOW_FIRST, read with the launch plan when the context is created)
    c->window_first = lim && n && c->plan.n_pools && c->plan.window_lds_bytes && !dump && c->stop_after == 0 && !c->no_window && total_bytes >= (uint64_t)lim * n;
    // Dense lattices: when four reservations of the learnt size (LDS bytes per input byte, steered by the redo rate: kgpu_ctx_sync) do not fit the pool, the
    // batch's pool workgroups get THREE wavefronts -- a fourth sentence would only wait for pages (the dense-lattice dictionary, natural density N/C = 8.6:
    // 57.8 -> 62.2 M sentences/s; cfg 2's reservations fit and it stays at four: three would cost it 21 %; profiles/experiments/r06_tile_sweep.txt)
    {
        const uint64_t est1 = n ? ((total_bytes / n) * c->dict->est_q8.load(std::memory_order_relaxed) >> 8) + 768u : 0u;
        c->roomy = n && c->plan.n_pools && c->plan.pool_limit_auto && c->plan.pool_waves[0] == 4 && 4u * est1 * 100u > (uint64_t)c->plan.pool_bytes[0] * 92u;
    }
    if (c->own_stream) { c->h2d_queued = false; return KGPU_OK; }
    hipStream_t want = c->short_stream;
    // ... and so does a pool-first chain whose last batch sent an eighth or more of its sentences on to the windowed kernel: its launches behind the pool
    // kernel are the long ones (cfg 3 in batches of 4096: 15.4 -> 17.5 M sentences/s on eight streams; a pool-ONLY chain loses there: cfg 2 101 -> 86)
    if ((c->window_first || c->long_share) && planned_long_streams()) {
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

static int enqueue(kgpu_ctx *c, const BatchArgs &a) {
    // The Control block is zero here: the previous launch's scan kernel left it so.
    if (c->ctl_dirty) HIPCHECK(hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream));
    c->ctl_dirty = true;  // until this enqueue is through
    hipEvent_t e0 = nullptr, ef = nullptr, e1 = nullptr, e2 = nullptr;
    int rc;
    const bool timed = c->profiling && (c->launch_seq++ % c->event_every) == 0;
    if (timed) {
        if ((rc = next_event(c, &e0)) || (rc = next_event(c, &ef)) || (rc = next_event(c, &e1)) || (rc = next_event(c, &e2))) return rc;
        HIPCHECK(hipEventRecord(e0, c->stream));
    }
    if (a.n) {
        const int pools_now = (c->window_first && !c->no_window) ? 0 : c->dict->big_pool_batches.load(std::memory_order_relaxed) > 0 ? c->plan.n_pools : std::min(c->plan.n_pools, 1);
        c->last_pools = pools_now;
        // The windowed kernel is in the chain while recent batches left the pools sentences (starts armed) -- an empty launch of a few thousand
        // workgroups behind a chip full of long-running wavefronts is not free -- or always, without a pool kernel in front of it.
        const bool window_now = c->plan.window_lds_bytes && !c->no_window && !a.dump_lattice && c->stop_after == 0 &&
                                (pools_now == 0 || c->dict->window_batches.load(std::memory_order_relaxed) > 0);
        c->last_window = window_now;
        // The general kernel closes the chain when nothing else is in it, in ablation / dump runs, and while recent batches left it sentences;
        // otherwise nothing does -- a sentence that needed more shows in the last work list's count, and kgpu_ctx_sync launches what is missing
        // over that list.
        c->last_tail = (pools_now == 0 && !window_now) || c->stop_after != 0 || a.dump_lattice || c->no_window ||
                       c->dict->tail_batches.load(std::memory_order_relaxed) > 0;
        // Two wavefronts per sentence (the windowed kernel's team form) when the list is short against the chip: the sentences of this batch AND of the
        // window-first batches in flight lately are at most twice the form's resident workgroups -- a lone batch of 1000 documents fills a quarter of the
        // single-wavefront slots and each document is one wavefront's chain; with four or more such batches in flight the ordinary form is the better use of the LDS.
        const int team_mode = c->plan.window_team_mode;   // KGPU_WINDOW_TEAM: 0 never, 2 whenever possible, default by the load
        bool team_now = false;
        if (pools_now == 0 && window_now && c->plan.window_team_workgroups > 0 && team_mode != 0) {
            if (!c->counted_long) { c->counted_long = (int)std::min<uint64_t>(a.n, 1u << 30); c->dict->long_sentences_in_flight.fetch_add(c->counted_long, std::memory_order_relaxed); }
            const int cur = c->dict->long_sentences_in_flight.load(std::memory_order_relaxed), old = c->dict->long_peak.load(std::memory_order_relaxed);
            const int peak = std::max(cur, old - old / 8);
            c->dict->long_peak.store(peak, std::memory_order_relaxed);
            // measured on cfg 5 (1000 documents per batch, Mchar/s, ordinary / team form): 1 in flight 1084 / 1495, 2: 1957 / 2153, 4: 3376 / 2372, 8: 4145 / 2405
            team_now = team_mode == 2 || peak <= 2 * c->plan.window_team_workgroups;
        }
        c->last_team = team_now;
        // The pool's SHAPE for this batch.  A pool-only chain keeps four wavefronts on 40 KB (cfg 2 100.9 M sentences/s; two on 20 KB: 98.4-99.3, the dense dictionary
        // 53.7 -> 50.8).  A chain that holds a windowed launch shares the chip with thousands of 10 KB single-wavefront workgroups that run for a millisecond: a
        // workgroup of two wavefronts on 20 KB finds its LDS and its wavefront slots far sooner than one of four on 40 KB -- cfg 3 at 4096 per batch 18.5 -> 21.9 M
        // sentences/s, at 65 536 23.9 -> 25.3 -- and in small batches (one sentence per wavefront slot: the pool launch lasts as long as its longest sentence) it
        // routes a little earlier (56 of its 64 pages of 312 B instead of all).  profiles/experiments/r05_long_chains.txt, sections 5 and 8.
        LaunchPlan pl = c->plan;
        if (pools_now > 0 && c->long_share && pl.pool_limit_auto && pl.alt_pool_workgroups > 0) {
            pl.pool_bytes[0] = pl.alt_pool_bytes; pl.pool_waves[0] = pl.alt_pool_waves; pl.pool_workgroups[0] = pl.alt_pool_workgroups;
            pl.pool_max_pages[0] = a.n <= 4u * 4096u ? 56u : 64u;
        }
        else if (pools_now > 0 && c->roomy) pl.pool_waves[0] = 3;   // (the same pools, the same grid: a workgroup's tickets hand its share out to three wavefronts)
        // The windowed launch behind the pools: as many workgroups as the last batch's share of routed sentences suggests (+ a quarter), not the chip's 4096 -- the
        // list is strided, so an estimate that is too small only makes a workgroup take a second sentence (the context's first batch gets the full grid).
        int window_grid = 0;
        if (pools_now > 0 && window_now && c->rt.batches > 0)
            window_grid = (int)std::min<uint64_t>(1u << 20, std::max<uint64_t>(256, ((a.n * c->win_share_q8) >> 8) * 5 / 4 + 64));
        hipError_t e = (hipError_t)launch_tokenize(c->dict->view, a, pl, pools_now, c->stop_after, c->stream, ef, window_now, c->last_tail, team_now, window_grid);
        if (e != hipSuccess) { set_error("k_tokenize launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    } else if (timed) HIPCHECK(hipEventRecord(ef, c->stream));
    // (the two small kernels behind a pool-only chain on a partner stream of each shared stream, so that the shared stream goes on with the next pool launch at once:
    // measured with 16 hardware queues, cfg 2 100.5 -> 72.9 M sentences/s -- whatever lets a fifth pool launch start early loses, profiles/experiments/r05_long_chains.txt)
    if (timed) HIPCHECK(hipEventRecord(e1, c->stream));
    {
        c->h_ctl->pack_overflow = 0;  // set by the compaction's workgroups in the host copy directly; this context's previous batch has been synced
        const bool small_wgs = a.n && c->last_window && (c->last_pools == 0 || c->long_share);   // (behind chains with a windowed launch)
        hipError_t e = (hipError_t)launch_scan_compact(a, c->h_ctl_dev, c->stream, small_wgs);
        if (e != hipSuccess) { set_error("scan/compact launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    }
    if (timed) HIPCHECK(hipEventRecord(e2, c->stream));
    HIPCHECK(hipEventRecord(c->done_ev, c->stream));
    c->ctl_dirty = false;
    c->last = a;
    c->pending = true;
    return KGPU_OK;
}

int kgpu::tokenize_device_impl(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
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
    if ((rc = ctx_pick_chain(c, n, total_bytes, false))) return rc;
    if ((rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)(total_bytes + n + 1) * sizeof(kgpu_token) + 64)) ||
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
    a.est_q8 = c->dict->est_q8.load(std::memory_order_relaxed);
    for (int k = 0; k < 4; ++k) a.ovf[k] = (uint32_t *)c->ovf.p + (size_t)k * (n + 1);
    return enqueue(c, a);
}

// The long-sentence kernel alone over work list `li` of the pending batch (which the chain left unserved), then scan + compaction again.
static int enqueue_tail(kgpu_ctx *c, int li) {
    const BatchArgs &a = c->last;
    // (the scan kernel zeroed the control block after publishing it; the completed batch is behind us on the stream)
    HIPCHECK(hipMemcpyAsync(&c->d_ctl->ovf_count[li], &c->tail_count, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    c->ctl_dirty = true;
    const bool window_was_in = c->last_window;
    hipError_t e = (hipError_t)launch_tail_only(c->dict->view, a, c->plan, li, window_was_in || c->no_window, c->stream);
    if (e != hipSuccess) { set_error("tail launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    if (!window_was_in && !c->no_window && c->plan.window_lds_bytes) c->last_window = true;
    c->last_tail = true;
    c->h_ctl->pack_overflow = 0;
    e = (hipError_t)launch_scan_compact(a, c->h_ctl_dev, c->stream);
    if (e != hipSuccess) { set_error("scan/compact launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    HIPCHECK(hipEventRecord(c->done_ev, c->stream));
    c->ctl_dirty = false;
    c->pending = true;
    return KGPU_OK;
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

// The pending batch is over (completed or given up): the context is free, its share of the dictionary's long sentences in flight is returned.
static void ctx_retire(kgpu_ctx *c) {
    c->pending = false;
    if (c->counted_long) { c->dict->long_sentences_in_flight.fetch_sub(c->counted_long, std::memory_order_relaxed); c->counted_long = 0; }
}

extern "C" int kgpu_ctx_sync(kgpu_ctx *c, uint64_t *n_tokens) {
    if (!c) { set_error("kgpu_ctx_sync: null ctx"); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(c->dict->device));
    for (;;) {
        if (!c->pending) { if (n_tokens) *n_tokens = 0; return KGPU_OK; }
        HIPCHECK(hipEventSynchronize(c->done_ev));  // this context's batch only: later work on a shared stream is not waited for
        if (c->h_ctl->window_fail && !c->h_ctl->arena_overflow && !c->no_window) {
            // the windowed kernel met a sentence it cannot hold and had no list to hand it on to: the batch once more without it
            c->no_window = true;
            c->rt.window_reruns++;
            // the rerun counts everything again: drop what this run left in the per-wavefront slots
            if (c->last.stat_slots) HIPCHECK(hipMemsetAsync(c->last.stat_slots, 0, (size_t)STAT_SLOTS * STAT_WORDS * 8, c->stream));
            c->tail_pass = false;
            int rc = enqueue(c, c->last);
            c->no_window = false;
            if (rc) { ctx_retire(c); return rc; }
            continue;
        }
        const int li_last = c->last_pools - 1 + (c->last_window ? 1 : 0) + (c->last_team ? 1 : 0);   // the list the chain ended on
        if (!c->last_tail && c->last.n && li_last >= 0 && !c->h_ctl->arena_overflow && c->h_ctl->ovf_count[li_last] > 0) {
            // The chain ended without its tail and a sentence needed it: ONLY what is missing (the windowed kernel if it was not in the chain,
            // then the general kernel), over the last work list (still in device memory; its length goes back into the control block the scan
            // kernel zeroed), then scan + compaction once more.  The pool kernel's work is not repeated: a corpus with a sparse but steady
            // share of long sentences pays a small launch per such batch, not the batch twice.  What the first pass counted (routing,
            // estimate feedback, work counters) is kept and merged below.
            c->rt.tail_reruns++;
            c->tail_saved = *c->h_ctl;
            c->tail_pass = true;
            c->tail_li = li_last;
            c->tail_had_window = c->last_window;
            c->tail_count = c->h_ctl->ovf_count[li_last];
            int rc = enqueue_tail(c, li_last);
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
            c->tail_pass = false;  // (the whole batch runs again: nothing of an earlier pass is merged)
            // the rerun counts everything again: drop what the aborted run left in the per-wavefront slots (ctl->work went with the control block)
            if (a.stat_slots) HIPCHECK(hipMemsetAsync(a.stat_slots, 0, (size_t)STAT_SLOTS * STAT_WORDS * 8, c->stream));
            if ((rc = enqueue(c, a))) { ctx_retire(c); return rc; }
            continue;
        }
        break;
    }
    ctx_retire(c);
    bool first_window = c->last_window, first_tail = c->last_tail;   // what the FIRST pass of this batch had in its chain (the arming below decays on that)
    if (c->tail_pass) {   // the published block is the tail pass's: put back what the first pass had counted
        c->tail_pass = false;
        first_window = c->tail_had_window; first_tail = false;
        Control &h = *c->h_ctl;
        const Control &sv = c->tail_saved;
        for (int k = 0; k < 4; ++k) { if (k <= c->tail_li) h.ovf_count[k] = sv.ovf_count[k]; h.late_count[k] += sv.late_count[k]; }   // lists up to the one the tail served are the first pass's
        for (int k = 0; k < 7; ++k) h.work[k] += sv.work[k];
        for (int k = 0; k < 10; ++k) h.phase[k] += sv.phase[k];
        h.pack_overflow |= sv.pack_overflow;
    }
    c->rt.batches++; c->rt.sentences += c->last.n;
    for (int k = 0; k < 4; ++k) { c->rt.deferred[k] += c->h_ctl->ovf_count[k]; c->rt.redone[k] += c->h_ctl->late_count[k]; }
    if (c->last_window && c->last.n) c->rt.long_launches++;
    if (c->last.n && c->last_pools > 0) {
        // arming of the launches behind the pools: what the pools left arms the windowed kernel, what the windowed kernel left arms the general
        // kernel; eight clean batches disarm (a wrong guess costs one small extra launch over the batch's last list, not the batch)
        const unsigned pool_left = c->h_ctl->ovf_count[c->last_pools - 1];
        if (c->plan.window_lds_bytes) {
            if (pool_left > 0) c->dict->window_batches.store(64, std::memory_order_relaxed);
            else if (first_window) c->dict->window_batches.fetch_sub(8, std::memory_order_relaxed);
        }
        if (c->last_window || !c->plan.window_lds_bytes) {   // (a batch whose pools left sentences while the windowed kernel was disarmed re-arms that one, not this)
            const unsigned behind = c->last_window ? c->h_ctl->ovf_count[c->last_pools] : pool_left;   // what the last launch in front of the general kernel left
            if (behind > 0) c->dict->tail_batches.store(64, std::memory_order_relaxed);
            else if (first_tail) c->dict->tail_batches.fetch_sub(8, std::memory_order_relaxed);
        }
    }
    if (c->last.n && c->last_pools > 0) {
        c->win_share_q8 = c->plan.window_lds_bytes ? (uint32_t)std::min<uint64_t>(256, (uint64_t)c->h_ctl->ovf_count[c->last_pools - 1] * 256 / c->last.n) : 0u;
        c->long_share = c->long_share ? c->win_share_q8 >= 16 : c->win_share_q8 >= 32;   // (entered at an eighth, left below a sixteenth: a share that hovers around the limit does not flap between streams)
    }
    if (c->last.n && c->last_pools == 0 && c->last_window && c->plan.n_pools) {
        // a chain that started with the windowed kernel: what it left arms the general kernel behind it, as above
        if (c->h_ctl->ovf_count[c->last_team ? 1 : 0] > 0) c->dict->tail_batches.store(64, std::memory_order_relaxed);
        else if (first_tail) c->dict->tail_batches.fetch_sub(8, std::memory_order_relaxed);
    }
    if (c->last.n && c->plan.n_pools && c->last_pools > 0) {
        // The pool kernel reserves est LDS bytes per input byte up front: a reservation that proves
        // too small costs a redo (late_count), one that is too large only idles pages until the
        // lattice is known -- steer for a redo rate of 1-3 %.  Applied to the value the batch ran with; races between
        // contexts only lose an adjustment.
        if (c->plan.n_pools > 1) {
            if (c->h_ctl->ovf_count[0] > 0) c->dict->big_pool_batches.store(64, std::memory_order_relaxed);
            else if (c->last_pools > 1) c->dict->big_pool_batches.fetch_sub(1, std::memory_order_relaxed);
        }
        const unsigned late = c->h_ctl->late_count[0];
        uint32_t est = c->last.est_q8;
        if ((uint64_t)late * 4 > c->last.n) est += est / 4;
        else if ((uint64_t)late * 32 > c->last.n) est += est / 16;
        else if ((uint64_t)late * 100 < c->last.n) est -= est / 128;
        est = std::min<uint32_t>(std::max<uint32_t>(est, 16 * 256), 1024 * 256);
        if (est != c->last.est_q8) c->dict->est_q8.store(est, std::memory_order_relaxed);
    }
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
    std::lock_guard<std::mutex> g(d->pool_mu);
    d->pool.push_back(c);
}

// A host-buffer path's copy of a batch's input, queued on the context's stream in front of the batch: the flag makes ctx_pick_chain order the
// batch behind it if the batch goes to another stream.
int kgpu::ctx_h2d(kgpu_ctx *c, void *dst, const void *src, size_t bytes, const char *what) {
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
    kgpu_ctx *c = nullptr;
    int rc = pool_get(d, &c);
    if (rc) return rc;
    // (the copies below go on c->stream, where the dump's own launch follows: no ctx_pick_chain, so no h2d_queued -- and none left behind)
    auto give_back = [&]() { c->h2d_queued = false; pool_put(d, c); };
    const uint64_t offs[2] = {0, len};
    Control hc{};
    if ((c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) ||
        (rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)(len + 2) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure(8)) || (rc = c->in_utf8.ensure((size_t)len + 16)) || (rc = c->in_off.ensure(16)) ||
        (rc = c->out_status.ensure(16))) { give_back(); return rc; }
    auto fail = [&](hipError_t e, const char *what) { set_error("kgpu_lattice_dump: %s: %s", what, hipGetErrorString(e)); c->ctl_dirty = true; give_back(); return KGPU_ERR_HIP; };
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
        if (want > ARENA_MAX) { set_error("scratch arena exceeded %zu bytes", ARENA_MAX); give_back(); return KGPU_ERR_INTERNAL; }
        if ((rc = c->arena.ensure(want))) { give_back(); return rc; }
    }
    if (!hc.dump[5]) { set_error("kgpu_lattice_dump: the sentence is not valid UTF-8"); give_back(); return KGPU_ERR_INVALID_ARG; }
    const uint64_t B = hc.dump[2], C = hc.dump[3], N = hc.dump[4], na = B + 4;
    std::vector<uint32_t> cbyte(C + 1), boff(C + 2), pre(N);
    std::vector<uint32_t> nodeA(4 * N), bucket(4 * N), nodeB(2 * N);
    const uint8_t *sa = (const uint8_t *)c->arena.p + hc.dump[0], *sn = (const uint8_t *)c->arena.p + hc.dump[1];
    // slab layouts: k_tokenize_general (kgpu_kernels.hip): cbyte | uspan | nb | boff | ... (u32[na] each); nodeA | bucket | nodeB | pre
    if ((e = hipMemcpy(cbyte.data(), sa, (C + 1) * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(boff.data(), sa + 3 * na * 4, (C + 2) * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(nodeA.data(), sn, N * 16, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(bucket.data(), sn + N * 16, N * 16, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(nodeB.data(), sn + N * 32, N * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(pre.data(), sn + N * 40, N * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "slab read-back");
    give_back();
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
        nd.dp = A[2] == 0xFFFFFFFFu ? (int32_t)hc.dump[6] : (int32_t)bucket[4 * A[2]];
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
