// kanpyo_amd/csrc/kgpu_chain.cpp -- the launch-chain policy (kgpu_chain.h): the plan of a context, the chain of a batch, its tail and the
// feedback from its outcome.  Plain host C++: no HIP, no device state.
#include "kgpu_chain.h"

#include <algorithm>
#include <cstdlib>

namespace kgpu {

unsigned pick_stream(const std::atomic<uint64_t> *load, unsigned n, std::atomic<unsigned> &cursor) {
    if (n <= 1) return 0;
    const unsigned from = cursor.load(std::memory_order_relaxed) % n;
    unsigned best = from;
    uint64_t least = load[from].load(std::memory_order_relaxed);
    for (unsigned k = 1; k < n && least; ++k) {   // (an empty stream at the cursor: nothing beats it)
        const unsigned i = (from + k) % n;
        const uint64_t l = load[i].load(std::memory_order_relaxed);
        if (l + l / STREAM_TIE_SHARE < least) { least = l; best = i; }   // (lighter by more than the tie band: see kgpu_chain.h)
    }
    cursor.store((best + 1) % n, std::memory_order_relaxed);
    return best;
}

LaunchPlan make_launch_plan(int cus, const Occupancy &occ) {
    LaunchPlan t{};
    t.general_workgroups = cus * 2;  // the last resort is rarely needed: few workgroups, so that an empty launch drains quickly on a busy chip
    // Default: four 40 KB pools per CU with 4 wavefronts each (16 sentences in flight per CU, any mix of
    // sizes).  A workgroup holds its LDS until its last wavefront is through, and the next launch's workgroups
    // start only then: four-wavefront workgroups drain sooner at the tail of a 4096-sentence batch than eight-
    // or sixteen-wavefront ones (80:8 66.3, 160:16 63.9, 40:4 68.6 M sentences/s; two-wavefront pools lose to
    // fragmentation, and any shape that is not 16 wavefronts per CU loses to the batch size: 4096 = 256 x 16).
    // A sentence expected to need more than 40 of a pool's 64 pages (25 KB, ~155 chars) goes to the
    // long-sentence kernel instead: LDS x time grows with the square of the length, and a few long sentences
    // would otherwise hold the pools while the short ones wait (cfg 3 in batches of 16384, M sentences/s by this limit:
    // 16 pages 16.3, 24 16.8, 32 17.6-18.4, 40 17.8-18.8, 48 17.1-18.4; round 2, batches of 4096: 56 11.6, 64 10.7 against 12.3; cfg 2 is
    // indifferent: 96.8-97.2 at 40, 96.4-97.0 at 48).
    // KGPU_POOL="<KiB>:<wavefronts>[:<max pages>][,...]", "0" = none.
    const char *e = getenv("KGPU_POOL");
    t.pool_limit_auto = e == nullptr;
    for (const char *q = e ? e : "40:4:32"; *q && t.n_pools < 2;) {
        int kib = atoi(q), w = 8, mp = 64;
        const char *c = q;
        while (*c && *c != ',' && *c != ':') ++c;
        if (*c == ':' && atoi(c + 1) > 0) {
            w = atoi(c + 1);
            ++c;
            while (*c && *c != ',' && *c != ':') ++c;
            if (*c == ':' && atoi(c + 1) > 0) mp = atoi(c + 1);
        }
        w = std::min(w, 16);
        mp = std::min(mp, 64);
        const int per_cu = kib >= 8 && kib <= 160 ? occ.pool((uint32_t)kib * 1024, (uint32_t)w) : 0;
        if (per_cu > 0) {
            t.pool_bytes[t.n_pools] = (uint32_t)kib * 1024; t.pool_waves[t.n_pools] = (uint32_t)w;
            t.pool_max_pages[t.n_pools] = (uint32_t)mp;
            t.pool_workgroups[t.n_pools] = cus * per_cu;
            ++t.n_pools;
        }
        while (*q && *q != ',') ++q;
        if (*q == ',') ++q;
    }
    t.alt_pool_bytes = 20 * 1024; t.alt_pool_waves = 2;
    const int alt_per_cu = (t.pool_limit_auto && t.n_pools) ? occ.pool(t.alt_pool_bytes, t.alt_pool_waves) : 0;
    t.alt_pool_workgroups = alt_per_cu > 0 ? cus * alt_per_cu : 0;
    // windowed kernel (everything the pools route away): KGPU_WINDOW="<KiB>" of LDS per single-wavefront workgroup, "0" = off (the general kernel then serves it all)
    const char *w = getenv("KGPU_WINDOW");
    int kib = w ? atoi(w) : 10;   // 10 KB: 16 workgroups per CU = the four wavefronts per SIMD its 128 VGPRs allow (round 4, after big buckets lost their pair tables: cfg 3 22.5 M sentences/s against 19.2 at 12 KB and 20.8 at 11, cfg 5 2.67 against 2.71 Gchar/s)
    if (kib < 8 || kib > 160) kib = 0;
    t.window_lds_bytes = (uint32_t)kib * 1024;
    const int per_cu = kib ? occ.window(t.window_lds_bytes) : 0;
    t.window_workgroups = cus * per_cu;
    if (per_cu <= 0) t.window_lds_bytes = 0;
    t.window_team_workgroups = t.window_lds_bytes ? cus * std::max(0, occ.window_team(t.window_lds_bytes)) : 0;
    const char *tm = getenv("KGPU_WINDOW_TEAM");
    t.window_team_mode = tm ? atoi(tm) : -1;
    const char *wf = getenv("KGPU_WINDOW_FIRST");
    t.window_first_bytes = (uint32_t)std::max(0, wf ? atoi(wf) : 1024);
    return t;
}

int Chain::pools() const {
    int k = 0;
    while (k < n && steps[k].kernel == Kernel::Pool) ++k;
    return k;
}
const Step *Chain::find(Kernel k) const {
    for (int i = 0; i < n; ++i) if (steps[i].kernel == k) return &steps[i];
    return nullptr;
}

// A batch of long sentences (by its average length: the host knows n and the bytes, not the lengths) starts with the windowed kernel -- the pool
// launch in front of it would only route: a thousand 40 KB workgroups that each look at four sentences and pass them on, waiting for LDS on a chip
// full of single-wavefront workgroups (cfg 5, 8 in flight: 2.97 -> 3.40 Gchar/s without it; profiles/experiments/r05_long_chains.txt).
bool starts_with_window(const LaunchPlan &plan, const Batch &b) {
    const uint64_t lim = plan.window_first_bytes;
    return lim && b.n && plan.n_pools && plan.window_lds_bytes && !b.dump && b.stop_after == 0 && !b.no_window && b.bytes >= lim * b.n;
}

// The windowed kernel over list `in` (-1: the identity); grid_est > 0: the host's estimate of that list's length.
static Step window_step(const LaunchPlan &plan, uint64_t n, int in, int out, int grid_est) {
    uint64_t wg = plan.window_workgroups;
    if (in < 0 && n < wg) wg = n;
    // behind the pools the list's length is on the device; a grid of the chip's full size is mostly workgroups that find nothing -- and each of them has to find a free
    // slot on a chip full of long-running wavefronts before it can say so, which is what the launch (and the scan behind it) then waits for: the host's estimate instead
    if (in >= 0 && grid_est > 0 && (uint64_t)grid_est < wg) wg = (uint64_t)grid_est;
    // more sentences expected than workgroups: they are claimed one by one instead of every G-th being a workgroup's (kgpu_window.hip)
    const uint64_t expected = in >= 0 ? (grid_est > 64 ? ((uint64_t)grid_est - 64) * 4 / 5 : 0) : n;
    return Step{Kernel::Window, in, out, (int)(wg ? wg : 1), plan.window_lds_bytes, 1, 0, expected > wg};
}
static Step general_step(const LaunchPlan &plan, uint64_t n, int in) {
    uint64_t wg = plan.general_workgroups;
    if (in < 0 && n < wg) wg = n;
    return Step{Kernel::General, in, -1, (int)(wg ? wg : 1), 0, 0, 0, false};
}

Chain build_chain(const LaunchPlan &plan, const Batch &b, Steering &st, ContextSteering &cs) {
    Chain ch;
    if (!b.n) return ch;
    const int pools = starts_with_window(plan, b) ? 0 : st.big_pool_batches.load(std::memory_order_relaxed) > 0 ? plan.n_pools : std::min(plan.n_pools, 1);
    // The windowed kernel is in the chain while recent batches left the pools sentences (starts armed) -- an empty launch of a few thousand
    // workgroups behind a chip full of long-running wavefronts is not free -- or always, without a pool kernel in front of it.
    const bool window = plan.window_lds_bytes && !b.no_window && !b.dump && b.stop_after == 0 &&
                        (pools == 0 || st.window_batches.load(std::memory_order_relaxed) > 0);
    // The general kernel closes the chain when nothing else is in it, in ablation / dump runs, and while recent batches left it sentences;
    // otherwise nothing does -- a sentence that needed more shows in the last work list's count, and the context runs tail_chain over that list.
    const bool general = (pools == 0 && !window) || b.stop_after != 0 || b.dump || b.no_window || st.tail_batches.load(std::memory_order_relaxed) > 0;
    // Two wavefronts per sentence (the windowed kernel's team form) when the list is short against the chip: the sentences of this batch AND of the
    // window-first batches in flight lately are at most twice the form's resident workgroups -- a lone batch of 1000 documents fills a quarter of the
    // single-wavefront slots and each document is one wavefront's chain; with four or more such batches in flight the ordinary form is the better use of the LDS.
    bool team = false;
    if (pools == 0 && window && plan.window_team_workgroups > 0 && plan.window_team_mode != 0) {
        if (!cs.counted_long) { cs.counted_long = (int)std::min<uint64_t>(b.n, 1u << 30); st.long_sentences_in_flight.fetch_add(cs.counted_long, std::memory_order_relaxed); }
        const int cur = st.long_sentences_in_flight.load(std::memory_order_relaxed), old = st.long_peak.load(std::memory_order_relaxed);
        const int peak = std::max(cur, old - old / 8);
        st.long_peak.store(peak, std::memory_order_relaxed);
        // measured on cfg 5 (1000 documents per batch, Mchar/s, ordinary / team form): 1 in flight 1084 / 1495, 2: 1957 / 2153, 4: 3376 / 2372, 8: 4145 / 2405
        team = plan.window_team_mode == 2 || peak <= 2 * plan.window_team_workgroups;
    }
    for (int k = 0; k < pools; ++k) {
        uint32_t bytes = plan.pool_bytes[k], waves = plan.pool_waves[k], pages = plan.pool_max_pages[k];
        uint64_t wg = plan.pool_workgroups[k];
        if (k == 0 && cs.long_share && plan.pool_limit_auto && plan.alt_pool_workgroups > 0) {
            // The pool's SHAPE for this batch.  A pool-only chain keeps four wavefronts on 40 KB (cfg 2 100.9 M sentences/s; two on 20 KB: 98.4-99.3, the dense dictionary
            // 53.7 -> 50.8).  A chain that holds a windowed launch shares the chip with thousands of 10 KB single-wavefront workgroups that run for a millisecond: a
            // workgroup of two wavefronts on 20 KB finds its LDS and its wavefront slots far sooner than one of four on 40 KB -- cfg 3 at 4096 per batch 18.5 -> 21.9 M
            // sentences/s, at 65 536 23.9 -> 25.3 -- and in small batches (one sentence per wavefront slot: the pool launch lasts as long as its longest sentence) it
            // routes a little earlier (56 of its 64 pages of 312 B instead of all).  profiles/experiments/r05_long_chains.txt, sections 5 and 8.
            bytes = plan.alt_pool_bytes; waves = plan.alt_pool_waves; wg = plan.alt_pool_workgroups;
            pages = b.n <= 4u * 4096u ? 56u : 64u;
        } else if (k == 0) {
            // Dense lattices: when four reservations of the learnt size (LDS bytes per input byte, steered by the redo rate: chain_feedback) do not fit the pool, the
            // batch's pool workgroups get THREE wavefronts -- a fourth sentence would only wait for pages (the dense-lattice dictionary, natural density N/C = 8.6:
            // 57.8 -> 62.2 M sentences/s; cfg 2's reservations fit and it stays at four: three would cost it 21 %; profiles/experiments/r06_tile_sweep.txt).
            // The same pools, the same grid: a workgroup's tickets hand its share out to three wavefronts.
            const uint64_t est1 = ((b.bytes / b.n) * b.est_q8 >> 8) + 768u;
            if (plan.pool_limit_auto && waves == 4 && 4u * est1 * 100u > (uint64_t)bytes * 92u) waves = 3;
        }
        const uint64_t want = (b.n + waves - 1) / waves;
        if (k == 0 && want < wg) wg = want;
        ch.steps[ch.n++] = Step{Kernel::Pool, k - 1, k, (int)(wg ? wg : 1), bytes, waves, pages, false};
    }
    ch.event_behind_first = pools > 0;
    if (window) {
        int in = pools - 1, grid_est = 0;
        if (team) {   // what that form cannot hold goes on to the ordinary form behind it, a small strided grid (it is rare)
            ch.steps[ch.n++] = Step{Kernel::WindowTeam, -1, 0, (int)std::min<uint64_t>(b.n, 1u << 30), plan.window_lds_bytes, 2, 0, false};
            in = 0; grid_est = 256;
        } else if (pools > 0 && b.share_known) {
            // behind the pools: as many workgroups as the last batch's share of routed sentences suggests (+ a quarter), not the chip's 4096 -- the list is
            // strided, so an estimate that is too small only makes a workgroup take a second sentence (the context's first batch gets the full grid)
            grid_est = (int)std::min<uint64_t>(1u << 20, std::max<uint64_t>(256, ((b.n * cs.win_share_q8) >> 8) * 5 / 4 + 64));
        }
        ch.steps[ch.n++] = window_step(plan, b.n, in, in + 1, grid_est);
    }
    if (general || ch.n == 0) ch.steps[ch.n++] = general_step(plan, b.n, ch.last_list());
    ch.small_scan = window && (pools == 0 || cs.long_share);
    ch.aux_one_launch = pools > 0 && !ch.small_scan && b.n <= AUX_ONE_LAUNCH_MAX;
    return ch;
}

// The windowed kernel over the list the chain ended on unless it was in the chain, then the general kernel over what is left.
Chain tail_chain(const LaunchPlan &plan, const Chain &ran) {
    Chain t;
    int li = ran.last_list();
    if (!ran.find(Kernel::Window) && plan.window_lds_bytes) { t.steps[t.n++] = window_step(plan, 0, li, li + 1, 0); ++li; }
    t.steps[t.n++] = general_step(plan, 0, li);
    return t;
}

void chain_feedback(const LaunchPlan &plan, const Chain &ran, const Chain *tail, const Control &h, uint64_t n, uint32_t est_q8, Steering &st,
                    ContextSteering &cs) {
    const int pools = ran.pools();
    if (!n) return;
    // arming of the launches behind the pools: what the pools left arms the windowed kernel, what the windowed kernel (or, without one, the pools)
    // left arms the general kernel; eight clean batches disarm (a wrong guess costs one small extra launch over the batch's last list, not the batch)
    const unsigned pool_left = pools ? h.ovf_count[pools - 1] : 0u;
    if (pools > 0 && plan.window_lds_bytes) {
        if (pool_left > 0) st.window_batches.store(64, std::memory_order_relaxed);
        else if (ran.find(Kernel::Window)) st.window_batches.fetch_sub(8, std::memory_order_relaxed);
    }
    // (a windowed launch of the tail pass counts: a batch whose pools left sentences while the windowed kernel was disarmed re-arms that one, not the general kernel)
    const Step *win = ran.find(Kernel::Window);
    if (!win && tail) win = tail->find(Kernel::Window);
    const int behind = win ? win->out : (pools > 0 && !plan.window_lds_bytes) ? pools - 1 : -1;   // the list of the last launch in front of the general kernel
    if (behind >= 0 && plan.n_pools) {
        if (h.ovf_count[behind] > 0) st.tail_batches.store(64, std::memory_order_relaxed);
        else if (ran.find(Kernel::General)) st.tail_batches.fetch_sub(8, std::memory_order_relaxed);
    }
    if (pools == 0) return;
    cs.win_share_q8 = plan.window_lds_bytes ? (uint32_t)std::min<uint64_t>(256, (uint64_t)pool_left * 256 / n) : 0u;
    cs.long_share = cs.long_share ? cs.win_share_q8 >= 16 : cs.win_share_q8 >= 32;   // (entered at an eighth, left below a sixteenth: a share that hovers around the limit does not flap between streams)
    // The pool kernel reserves est LDS bytes per input byte up front: a reservation that proves too small costs a redo (late_count), one that is
    // too large only idles pages until the lattice is known -- steer for a redo rate of 1-3 %.  Applied to the value the batch ran with.
    if (plan.n_pools > 1) {
        if (h.ovf_count[0] > 0) st.big_pool_batches.store(64, std::memory_order_relaxed);
        else if (pools > 1) st.big_pool_batches.fetch_sub(1, std::memory_order_relaxed);
    }
    const unsigned late = h.late_count[0];
    uint32_t est = est_q8;
    if ((uint64_t)late * 4 > n) est += est / 4;
    else if ((uint64_t)late * 32 > n) est += est / 16;
    else if ((uint64_t)late * 100 < n) est -= est / 128;
    est = std::min<uint32_t>(std::max<uint32_t>(est, 16 * 256), 1024 * 256);
    if (est != est_q8) st.est_q8.store(est, std::memory_order_relaxed);
}

}  // namespace kgpu
