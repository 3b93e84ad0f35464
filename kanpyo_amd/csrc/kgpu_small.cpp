// kanpyo_amd/csrc/kgpu_small.cpp -- kgpu_tokenize_batch's small calls: at most SMALL_MAX_N sentences / SMALL_MAX_BYTES in ONE launch.
//
// Owns: the single-launch small call, the combiner that lets concurrent small calls share a launch (its lock: kgpu_lock.h), the CPU
// budget and the futex helpers its waits use, the KGPU_SMALL_TRACE counters (kgpu_debug_small_*), and kgpu_debug_concurrent_callers.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <sched.h>
#include <string>
#include <sys/prctl.h>
#include <thread>
#include <vector>

#include "kgpu_lock.h"
#include "kgpu_runtime.h"

// ---- small calls: ONE launch, no copies ------------------------------------------------------------------
// The reference's call shape is one sentence per call (src/bin/kanpyo.rs:106-126); the general path costs such a call
// five dependent launches, two host-to-device and three device-to-host copies (~120 us).  Here the sentences and the
// results live in one pinned, device-mapped block: the pool kernel reads its input over PCIe, tokenizes one sentence
// per wavefront, compacts and publishes by itself (kgpu_pool.hip, `fused_host`), and the host polls a sequence number.
static constexpr uint64_t SMALL_MAX_N = 128, SMALL_MAX_BYTES = 16 * 1024;
static constexpr size_t SM_OFF_OFFS = SMALL_MAX_BYTES + 64, SM_OFF_TOK = SM_OFF_OFFS + (SMALL_MAX_N + 1) * 8 + 56,
                        SM_OFF_TOFF = SM_OFF_TOK + (SMALL_MAX_BYTES + SMALL_MAX_N) * sizeof(kgpu_token),
                        SM_OFF_STATUS = SM_OFF_TOFF + (SMALL_MAX_N + 1) * 8 + 56, SM_BYTES = SM_OFF_STATUS + SMALL_MAX_N + 64;

// One caller's part of a single-launch small call.
struct SmallReq {
    const uint8_t *utf8; const uint64_t *offsets; uint64_t n;
    kgpu_token *tokens; uint64_t token_capacity; uint64_t *tok_offsets; uint8_t *status; uint64_t *n_tokens;
    int rc = -1;              // KGPU_OK: done; KGPU_ERR_CAPACITY: done, this caller's buffer too small; -1: not served here (a sentence needs the long way)
    char err[160] = "";       // the message behind rc (set_error is thread-local: the caller's thread repeats it)
    bool done = false;
};

// The launch for one or more callers' sentences (`reqs` in arrival order; together at most SMALL_MAX_N sentences / SMALL_MAX_BYTES).
// Returns KGPU_OK when the launch itself went through (every request then has its own rc), else the error (no request was served).
// KGPU_SMALL_TRACE=1: where a small call's wall time goes, summed over the process (microseconds): kgpu_debug_small_trace reads and resets
static std::atomic<uint64_t> g_st[8];  // launches, prep ns, launch-call ns, poll ns, hand-out ns, sentences
static inline uint64_t now_ns() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec; }
extern "C" void kgpu_debug_small_trace(uint64_t out[8]) { for (int k = 0; k < 8; ++k) out[k] = g_st[k].exchange(0); }
// ... and where the callers' CPU time goes (CLOCK_THREAD_CPUTIME_ID at the phase boundaries, ns summed over all threads): [0] calls that joined a batch,
// [1] calls that led one, [2] entry + the combiner's lock, [3] a follower's wait, [4] the leader's window, [5] close + context, [6] assembling the launch,
// [7] the launch call, [8] the poll, [9] handing the records out, [10] waking the followers, [11] hipSetDevice at the entry point
std::atomic<uint64_t> kgpu::g_sc[16];
uint64_t kgpu::cpu_ns() { timespec t; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t); return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec; }
bool kgpu::small_trace_on() { static const bool on = env_flag_now("KGPU_SMALL_TRACE"); return on; }
extern "C" void kgpu_debug_small_cpu(uint64_t out[16]) { for (int k = 0; k < 16; ++k) out[k] = g_sc[k].exchange(0); }

static unsigned cpu_budget();
static void short_sleep_us(unsigned us);
static int small_call(kgpu_dict *d, kgpu_ctx *c, SmallReq *const *reqs, size_t nreq) {
    const bool trace = small_trace_on();
    const uint64_t tt0 = trace ? now_ns() : 0, cc0 = trace ? cpu_ns() : 0;
    uint64_t n = 0, total = 0;
    for (size_t r = 0; r < nreq; ++r) { n += reqs[r]->n; total += reqs[r]->offsets[reqs[r]->n] - reqs[r]->offsets[0]; }
    int rc;
    if (!c->sm_host) {
        if (hipHostMalloc((void **)&c->sm_host, SM_BYTES, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void **)&c->sm_dev, c->sm_host, 0) != hipSuccess) {
            if (c->sm_host) { (void)hipHostFree(c->sm_host); c->sm_host = nullptr; }
            (void)hipGetLastError();
            return KGPU_OK;  // every request keeps rc = -1: the general path
        }
    }
    if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
    // (no scratch arena: this path launches the pool kernel alone, whose lattices live in LDS -- a context that only ever serves small calls holds no 256 MiB)
    if ((rc = c->stage.ensure((size_t)(total + n + 1) * sizeof(kgpu_token) + 64)) ||
        (rc = c->tok_count.ensure((size_t)(n + 1) * 4)) || (rc = c->ovf.ensure((size_t)(n + 1) * 4 * 4)))
        return rc;
    uint64_t *h_off = (uint64_t *)(c->sm_host + SM_OFF_OFFS);
    {
        uint64_t at = 0, si = 0;
        for (size_t r = 0; r < nreq; ++r) {
            const SmallReq &q = *reqs[r];
            const uint64_t base = q.offsets[0], bytes = q.offsets[q.n] - base;
            if (bytes) std::memcpy(c->sm_host + at, q.utf8 + base, (size_t)bytes);
            for (uint64_t i = 0; i < q.n; ++i) h_off[si + i] = at + (q.offsets[i] - base);
            at += bytes; si += q.n;
        }
        h_off[n] = at;
    }
    const uint32_t seq = ++c->sm_seq ? c->sm_seq : ++c->sm_seq;  // never 0
    __atomic_store_n(&c->h_ctl->small_flag, 0u, __ATOMIC_RELEASE);
    BatchArgs a{};
    a.utf8 = c->sm_dev; a.offsets = (const uint64_t *)(c->sm_dev + SM_OFF_OFFS); a.n = n; a.ctl = c->d_ctl;
    a.arena = (uint8_t *)c->arena.p; a.arena_bytes = c->arena.bytes;
    a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p;
    a.status = c->sm_dev + SM_OFF_STATUS; a.out = (kgpu_token *)(c->sm_dev + SM_OFF_TOK); a.out_cap = total + n;
    a.tok_offsets = (uint64_t *)(c->sm_dev + SM_OFF_TOFF);
    a.est_q8 = d->steer.est_q8.load(std::memory_order_relaxed);
    for (int k = 0; k < 4; ++k) a.ovf[k] = (uint32_t *)c->ovf.p + (size_t)k * (n + 1);
    a.fused_host = c->h_ctl_dev; a.fused_seq = seq;
    if (c->ctl_dirty) HIPCHECK(hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream));
    c->ctl_dirty = true;
    const uint64_t tt1 = trace ? now_ns() : 0, cc1 = trace ? cpu_ns() : 0;
    {
        hipError_t e = (hipError_t)launch_small_call(d->view, a, c->stream);
        if (e != hipSuccess) { set_error("small-call launch: %s", hipGetErrorString(e)); return KGPU_ERR_HIP; }
    }
    const uint64_t tt2 = trace ? now_ns() : 0, cc2 = trace ? cpu_ns() : 0;
    // poll the sequence number (the kernel's last store); a stream query now and then catches a failed launch
    for (uint64_t spin = 0;; ++spin) {
        if (__atomic_load_n(&c->h_ctl->small_flag, __ATOMIC_ACQUIRE) == seq) break;
        if ((spin & 0xFFFF) == 0xFFFF) {
            hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(&c->h_ctl->small_flag, __ATOMIC_ACQUIRE) == seq) break;
                set_error("small call: the kernel finished without publishing"); return KGPU_ERR_INTERNAL;
            }
            if (q != hipErrorNotReady) { set_error("small call: %s", hipGetErrorString(q)); return KGPU_ERR_HIP; }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        // many callers inside the entry point: most of them need a CPU to assemble or pick up their results -- this thread's poll lets them have it;
        // more callers than CPUs: sleep through most of the launch's ~45 us instead (the poll costs the group's CPU quota, the sleep does not)
        if ((spin & 63) == 63) {
            const int callers = d->combiner_callers();
            if (callers > (int)cpu_budget()) short_sleep_us(spin < 64 ? 25 : 8);
            else if (callers > 8) sched_yield();
        }
    }
    const uint64_t tt3 = trace ? now_ns() : 0, cc3 = trace ? cpu_ns() : 0;
    struct TraceOut { bool on; uint64_t t0, t1, t2, t3, n, c0, c1, c2, c3; ~TraceOut() { if (on) { const uint64_t t4 = now_ns(), c4 = cpu_ns(); g_st[0] += 1; g_st[1] += t1 - t0; g_st[2] += t2 - t1; g_st[3] += t3 - t2; g_st[4] += t4 - t3; g_st[5] += n;
        g_sc[6] += c1 - c0; g_sc[7] += c2 - c1; g_sc[8] += c3 - c2; g_sc[9] += c4 - c3; } } } trace_out{trace, tt0, tt1, tt2, tt3, n, cc0, cc1, cc2, cc3};
    c->ctl_dirty = false;  // the publishing wavefront zeroed the device block
    c->rt.batches++; c->rt.sentences += n;
    c->rt.deferred[0] += c->h_ctl->ovf_count[0]; c->rt.redone[0] += c->h_ctl->late_count[0];
    c->rt.small_calls += nreq;
    if (nreq > 1) { c->rt.combined_calls += nreq; c->rt.combined_launches++; }
    if (c->h_ctl->ovf_count[0] != 0 || c->h_ctl->arena_overflow || c->h_ctl->small_abort) {  // a sentence left for the long / HBM-scratch kernels, or the rendezvous timed out
        c->rt.small_fallbacks += nreq;
        return KGPU_OK;  // rc = -1 everywhere: each caller takes the general path with its own sentences
    }
    const uint64_t *h_toff = (const uint64_t *)(c->sm_host + SM_OFF_TOFF);
    const kgpu_token *h_tok = (const kgpu_token *)(c->sm_host + SM_OFF_TOK);
    uint64_t si = 0;
    for (size_t r = 0; r < nreq; ++r) {   // every caller's dense slice
        SmallReq &q = *reqs[r];
        const uint64_t t0 = h_toff[si], got = h_toff[si + q.n] - t0;
        if (q.n_tokens) *q.n_tokens = got;
        if (got > q.token_capacity) {
            snprintf(q.err, sizeof q.err, "token buffer too small: need %llu, capacity %llu", (unsigned long long)got, (unsigned long long)q.token_capacity);
            q.rc = KGPU_ERR_CAPACITY;
        } else {
            if (got) std::memcpy(q.tokens, h_tok + t0, (size_t)got * sizeof(kgpu_token));
            for (uint64_t i = 0; i <= q.n; ++i) q.tok_offsets[i] = h_toff[si + i] - t0;
            if (q.status) std::memcpy(q.status, c->sm_host + SM_OFF_STATUS + si, (size_t)q.n);
            q.rc = KGPU_OK;
        }
        si += q.n;
    }
    return KGPU_OK;
}

// ---- the combiner: concurrent small calls share one launch -------------------------------------------------------------
// The reference's tokenize() takes &self and is Send + Sync (src/tokenizer.rs:16): a server calls it from many threads, one sentence
// per call (src/bin/kanpyo.rs:106-126).  A launch costs the same ~50 us whether it carries one sentence or a hundred, so callers that
// arrive while another small call is being assembled join it: the first one in is the leader -- it keeps the batch open for a short
// window (only while other callers are inside the entry point: a lone caller never waits), takes a pooled context, launches, and hands
// every follower its own dense slice back.  Followers sleep on a condition variable meanwhile.
struct Combiner {
    // A batch lives on the heap, shared by its leader and its followers (a follower may still be reading its own result when the leader returns).
    struct Batch {
        std::vector<SmallReq *> reqs; uint64_t n = 0, bytes = 0; bool closed = false;
        std::atomic<uint32_t> done{0};   // futex word: followers sleep on it, ONE wake-all syscall releases them (no shared condition variable: a
    };                                   // batch's completion wakes its own followers only, and nobody queues on a mutex to find out)
    // (each on a cache line of its own: every caller adds itself to `callers` on the way in and out, the lock's waiters read the lock word meanwhile)
    alignas(64) SpinLock mu;
    std::shared_ptr<Batch> open;
    alignas(64) std::atomic<int> callers{0};     // threads inside the small-call entry
    alignas(64) std::atomic<int> in_flight{0};   // launches between close and completion
};
int kgpu_dict::combiner_callers() const { return combiner ? combiner->callers.load(std::memory_order_relaxed) : 0; }
Combiner *kgpu::combiner_new() { return new Combiner(); }
void kgpu::combiner_delete(Combiner *c) { delete c; }
static Combiner &combiner_of(kgpu_dict *d) { return *d->combiner; }
static unsigned combine_window_us() {
    static const unsigned us = [] { const char *e = getenv("KGPU_COMBINE_US"); const int v = e ? atoi(e) : 12; return (unsigned)(v < 0 ? 0 : v > 1000 ? 1000 : v); }();
    return us;
}
static int combine_max_in_flight() {
    static const int v = [] { const char *e = getenv("KGPU_COMBINE_LAUNCHES"); const int x = e ? atoi(e) : 4; return x < 1 ? 1 : x > 64 ? 64 : x; }();
    return v;
}
// CPUs this process may actually use: hardware threads, narrowed by the affinity mask and the cgroup's CPU quota (cpu.max, or cfs_quota_us / cfs_period_us).
// With more callers inside the entry point than that, a spinning thread takes the CPU a sleeping caller needs -- and under a CFS quota the spinning burns the
// whole group's budget for the period (round 4: 128 threads on a 16-CPU quota, p99 64 ms) -- so the waits below sleep instead of spinning.
static unsigned cpu_budget() {
    static const unsigned n = [] {
        unsigned hw = std::thread::hardware_concurrency();
        if (!hw) hw = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) { const unsigned a = (unsigned)CPU_COUNT(&set); if (a && a < hw) hw = a; }
        long long quota = -1, period = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32];
            if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
            fclose(f);
        } else {
            if (FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%lld", &quota) != 1) quota = -1; fclose(fq); }
            if (FILE *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lld", &period) != 1) period = 0; fclose(fp); }
        }
        if (quota > 0 && period > 0) { const unsigned c = (unsigned)((quota + period - 1) / period); if (c && c < hw) hw = c; }
        if (const char *e = getenv("KGPU_CPU_BUDGET")) { const int v = atoi(e); if (v > 0) hw = (unsigned)v; }   // (tests: force the crowded mode)
        return hw;
    }();
    return n;
}
// A short sleep (the default 50 us timer slack would make 15 us into 65: the slack is lowered for the sleep and put back)
static void short_sleep_us(unsigned us) {
    const int slack = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
    if (slack > 2000) prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    timespec ts{0, (long)us * 1000};
    nanosleep(&ts, nullptr);
    if (slack > 2000) prctl(PR_SET_TIMERSLACK, (unsigned long)slack, 0, 0, 0);
}
static void futex_wait(std::atomic<uint32_t> *w, uint32_t expected) { syscall(SYS_futex, (uint32_t *)w, FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0); }
static void futex_wake_all(std::atomic<uint32_t> *w) { syscall(SYS_futex, (uint32_t *)w, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0); }

// KGPU_OK / KGPU_ERR_CAPACITY: served; -1: take the general path; other: error
static int small_call_combined(kgpu_dict *d, SmallReq &me) {
    Combiner &cb = combiner_of(d);
    const uint64_t my_bytes = me.offsets[me.n] - me.offsets[0];
    struct CallerCount { std::atomic<int> &c; CallerCount(std::atomic<int> &c_) : c(c_) { c.fetch_add(1, std::memory_order_acq_rel); } ~CallerCount() { c.fetch_sub(1, std::memory_order_acq_rel); } } in(cb.callers);
    std::shared_ptr<Combiner::Batch> mine;
    const bool trace = small_trace_on();
    uint64_t k0 = trace ? cpu_ns() : 0;
    for (;;) {   // (a batch is allocated OUTSIDE the lock -- the lock is held for a push_back and two additions -- and only by a caller that found none to join)
        {
            std::unique_lock<SpinLock> l(cb.mu);
            std::shared_ptr<Combiner::Batch> b = cb.open;
            if (b && !b->closed && b->n + me.n <= SMALL_MAX_N && b->bytes + my_bytes <= SMALL_MAX_BYTES) {   // join the batch being assembled
                b->reqs.push_back(&me); b->n += me.n; b->bytes += my_bytes;
                l.unlock();
                const uint64_t k1 = trace ? cpu_ns() : 0;
                while (b->done.load(std::memory_order_acquire) == 0) futex_wait(&b->done, 0);   // the leader has written my records and my rc before it sets the word
                if (trace) { g_sc[0] += 1; g_sc[2] += k1 - k0; g_sc[3] += cpu_ns() - k1; }
                if (me.rc > 0 && me.err[0]) set_error("%s", me.err);
                return me.rc;
            }
            if (mine) {
                mine->reqs.push_back(&me); mine->n = me.n; mine->bytes = my_bytes;
                cb.open = mine;   // (a batch another leader still holds open but that has no room for me stays its leader's: it closes it itself)
                break;
            }
        }
        mine = std::make_shared<Combiner::Batch>();
        mine->reqs.reserve(SMALL_MAX_N);   // (no reallocation under the lock later)
    }
    // Leader.  A lone caller launches at once.  With other callers inside the entry point the batch stays open for a short window -- and, when
    // the device already has its fill of small launches in flight, until one of them completes (or the batch is full): the batch size follows the
    // load (group commit), the number of launches per second stays what the streams carry.  Spinning: the waits are shorter than a futex sleep.
    if (trace) { const uint64_t k1 = cpu_ns(); g_sc[1] += 1; g_sc[2] += k1 - k0; k0 = k1; }
    const unsigned win = combine_window_us();
    if (win && cb.callers.load(std::memory_order_acquire) > 1) {
        timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
        for (;;) {
            if (cb.callers.load(std::memory_order_relaxed) > (int)cpu_budget()) short_sleep_us(10);   // more callers than CPUs: the window is slept, not spun
            else for (int k = 0; k < 16; ++k) {
#if defined(__x86_64__)
                __builtin_ia32_pause();
#endif
            }
            timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
            const long long us = (t1.tv_sec - t0.tv_sec) * 1000000ll + (t1.tv_nsec - t0.tv_nsec) / 1000;
            const bool busy = cb.in_flight.load(std::memory_order_acquire) >= combine_max_in_flight();
            if ((us >= (long long)win && !busy) || us >= 400) break;   // (a four times longer window when callers exceed CPUs: measured, 64 threads 358 -> 301 k sentences/s, 128 unchanged)
            std::lock_guard<SpinLock> g(cb.mu);
            if (mine->n >= SMALL_MAX_N || mine->bytes + 256 > SMALL_MAX_BYTES) break;  // full
            if (!busy && (int)mine->reqs.size() >= cb.callers.load(std::memory_order_acquire)) break;  // everyone who is here is in
        }
    }
    if (trace) { const uint64_t k1 = cpu_ns(); g_sc[4] += k1 - k0; k0 = k1; }
    {
        std::lock_guard<SpinLock> g(cb.mu);
        mine->closed = true;
        if (cb.open == mine) cb.open.reset();
    }
    cb.in_flight.fetch_add(1, std::memory_order_acq_rel);
    kgpu_ctx *c = nullptr;
    int rc = pool_get(d, &c);
    if (trace) { const uint64_t k1 = cpu_ns(); g_sc[5] += k1 - k0; k0 = k1; }
    if (!rc) {
        rc = c->plan.n_pools ? small_call(d, c, mine->reqs.data(), mine->reqs.size()) : KGPU_OK;
        pool_put(d, c);
    }
    cb.in_flight.fetch_sub(1, std::memory_order_acq_rel);
    const int my_rc = rc ? rc : me.rc;
    if (rc) for (SmallReq *q : mine->reqs) { q->rc = rc; snprintf(q->err, sizeof q->err, "%s", kgpu_last_error()); }
    const bool had_followers = mine->reqs.size() > 1;
    if (trace) k0 = cpu_ns();
    mine->done.store(1, std::memory_order_release);   // (followers may return -- and their SmallReq die -- from here on: nothing of theirs is touched below)
    if (had_followers) futex_wake_all(&mine->done);
    if (trace) g_sc[10] += cpu_ns() - k0;
    if (my_rc > 0 && !rc && me.err[0]) set_error("%s", me.err);
    return my_rc;
}

int kgpu::tokenize_small(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, kgpu_token *tokens, uint64_t token_capacity,
                         uint64_t *tok_offsets, uint8_t *status, uint64_t *n_tokens) {
    if (n < 1 || n > SMALL_MAX_N || offsets[n] - offsets[0] > SMALL_MAX_BYTES || test_hooks().no_small_calls) return -1;
    SmallReq me{utf8, offsets, n, tokens, token_capacity, tok_offsets, status, n_tokens};
    return small_call_combined(d, me);
}

// ---- measurement / test only (bench.py's concurrent_callers leg, tests/test_gpu_concurrent.py; not part of include/kanpyo_gpu.h): `threads` host
// threads call kgpu_tokenize_batch in a loop, thread t with n_pattern[t % n_pat] sentences per call (the reference's shape is 1: src/bin/kanpyo.rs:106-126),
// walking round the corpus from its own starting point.  With `expect_tokens` / `expect_offsets` (the whole corpus tokenized once, e.g. by the oracle)
// every call's records are compared: stats[4] counts the calls that differ.  stats: [0] wall seconds, [1] p50 / [2] p99 / [3] mean call latency in us,
// [4] mismatching calls, [5] calls made, [6] sentences tokenized.  Python threads cannot drive this: the GIL serialises what surrounds each call.
extern "C" int kgpu_debug_concurrent_callers(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n_sentences, int threads, int calls_per_thread,
                                             const int *n_pattern, int n_pat, const kgpu_token *expect_tokens, const uint64_t *expect_offsets, double *stats) {
    if (!d || !offsets || !n_sentences || threads < 1 || threads > 1024 || calls_per_thread < 1 || !n_pattern || n_pat < 1 || !stats) { set_error("kgpu_debug_concurrent_callers: bad argument"); return KGPU_ERR_INVALID_ARG; }
    std::vector<std::vector<float>> lat((size_t)threads);
    std::vector<uint64_t> bad((size_t)threads, 0), sent((size_t)threads, 0), cpu((size_t)threads, 0);   // cpu: the thread's own CPU time over its calls (ns)
    std::vector<int> rcs((size_t)threads, KGPU_OK);
    std::vector<std::string> errs((size_t)threads);
    // The start gate sleeps (a futex word), it does not spin: a hundred threads yielding in a loop while the rest are created burn, each on its own CPU of the
    // host, a good part of a 16-CPU cgroup quota's 100 ms period before the first call is made -- and the period's remainder is then spent throttled.
    std::atomic<int> ready{0};
    std::atomic<uint32_t> go{0};
    auto now_us = [] { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e6 + t.tv_nsec * 1e-3; };
    auto body = [&](int t) {
        const uint64_t npc = (uint64_t)std::max(1, n_pattern[t % n_pat]);
        uint64_t maxb = 0;
        for (uint64_t i = 0; i < n_sentences; ++i) maxb = std::max(maxb, offsets[i + 1] - offsets[i]);
        std::vector<kgpu_token> tok((size_t)(npc * (maxb + 1) + 8));
        std::vector<uint64_t> toff((size_t)npc + 1), off2((size_t)npc + 1);
        std::vector<uint8_t> st((size_t)npc + 1), text;
        lat[(size_t)t].reserve((size_t)calls_per_thread);
        uint64_t at = ((uint64_t)t * 7919u) % n_sentences;
        ready.fetch_add(1);
        while (go.load(std::memory_order_acquire) == 0) futex_wait(&go, 0);
        const uint64_t c0 = cpu_ns();
        struct CpuOut { uint64_t &out, c0; ~CpuOut() { out = cpu_ns() - c0; } } cpu_out{cpu[(size_t)t], c0};
        for (int k = 0; k < calls_per_thread; ++k) {
            if (at + npc > n_sentences) at = 0;
            const uint64_t m = std::min(npc, n_sentences - at);
            uint64_t got = 0;
            const double t0 = now_us();
            const int rc = kgpu_tokenize_batch(d, utf8, offsets + at, m, tok.data(), tok.size(), toff.data(), st.data(), &got);
            lat[(size_t)t].push_back((float)(now_us() - t0));
            if (rc) { rcs[(size_t)t] = rc; errs[(size_t)t] = kgpu_last_error(); return; }
            sent[(size_t)t] += m;
            if (expect_tokens && expect_offsets) {
                const uint64_t e0 = expect_offsets[at], en = expect_offsets[at + m] - e0;
                bool same = got == en && std::memcmp(tok.data(), expect_tokens + e0, (size_t)en * sizeof(kgpu_token)) == 0;
                for (uint64_t i = 0; same && i <= m; ++i) same = toff[(size_t)i] == expect_offsets[at + i] - e0;
                if (!same) bad[(size_t)t]++;
            }
            at += m;
        }
    };
    std::vector<std::thread> th;
    try { for (int t = 0; t < threads; ++t) th.emplace_back(body, t); }
    catch (...) { go.store(2); futex_wake_all(&go); for (auto &x : th) x.join(); set_error("kgpu_debug_concurrent_callers: could not start %d threads", threads); return KGPU_ERR_INTERNAL; }
    while (ready.load() < threads) short_sleep_us(50);
    const double t0 = now_us();
    go.store(1, std::memory_order_release);
    futex_wake_all(&go);
    for (auto &x : th) x.join();
    const double wall = (now_us() - t0) * 1e-6;
    for (int t = 0; t < threads; ++t) if (rcs[(size_t)t]) { set_error("%s", errs[(size_t)t].c_str()); return rcs[(size_t)t]; }
    std::vector<float> all;
    uint64_t nbad = 0, nsent = 0;
    for (int t = 0; t < threads; ++t) { all.insert(all.end(), lat[(size_t)t].begin(), lat[(size_t)t].end()); nbad += bad[(size_t)t]; nsent += sent[(size_t)t]; }
    std::sort(all.begin(), all.end());
    double mean = 0; for (float x : all) mean += x;
    stats[0] = wall; stats[1] = all[all.size() / 2]; stats[2] = all[(size_t)((double)all.size() * 0.99)]; stats[3] = mean / (double)all.size();
    stats[4] = (double)nbad; stats[5] = (double)all.size(); stats[6] = (double)nsent;
    { uint64_t c = 0; for (uint64_t x : cpu) c += x; stats[7] = (double)c * 1e-9; }   // CPU seconds of the calling threads, start gate and thread start-up left out
    return KGPU_OK;
}
