// The launch-chain policy (kanpyo_amd/csrc/kgpu_chain.cpp) on the CPU, no device: tests/test_chain_policy_cpu.py builds this file with g++ against
// kgpu_chain.cpp alone.  Every expected value is the one the code before the policy had its own module computed; "was X:N" cites that code at
// commit f121e16 (kgpu_ctx.cpp: the chain choice and the feedback, kgpu_kernels.hip: the launchers and the plan).  Prints "ok <checks>" or FAIL lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kanpyo_amd/csrc/kgpu_chain.h"

using namespace kgpu;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) { ++failures; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// fake occupancies: 40 KB x 4 -> 4 per CU, 20 KB x 2 -> 8, 80 KB x 8 -> 2, 160 KB x 4 -> 1; windowed 10 KB -> 16, its team form -> 3
static int pool_occ(uint32_t bytes, uint32_t waves) {
    if (bytes == 40 * 1024 && waves == 4) return 4;
    if (bytes == 20 * 1024 && waves == 2) return 8;
    if (bytes == 80 * 1024 && waves == 8) return 2;
    if (bytes == 160 * 1024 && waves == 4) return 1;
    return 0;
}
static int window_occ(uint32_t bytes) { return bytes == 10 * 1024 ? 16 : 0; }
static int team_occ(uint32_t bytes) { return bytes == 10 * 1024 ? 3 : 0; }
static const int CUS = 256;

static LaunchPlan plan_with(const char *pool, const char *window = nullptr, const char *team = nullptr) {
    pool ? setenv("KGPU_POOL", pool, 1) : unsetenv("KGPU_POOL");
    window ? setenv("KGPU_WINDOW", window, 1) : unsetenv("KGPU_WINDOW");
    team ? setenv("KGPU_WINDOW_TEAM", team, 1) : unsetenv("KGPU_WINDOW_TEAM");
    unsetenv("KGPU_WINDOW_FIRST");
    return make_launch_plan(CUS, Occupancy{pool_occ, window_occ, team_occ});
}

static Batch batch(uint64_t n, uint64_t bytes, bool share_known = true) { return Batch{n, bytes, 64 * 256, 0, false, false, share_known}; }

// Every chain this file builds goes through here: a Window / WindowTeam step always has a list to hand on to (out >= 0).  The windowed kernel's other
// way out -- no list: flag Control::window_fail, the host reruns the batch without it (kgpu_routing.window_reruns) -- is therefore never taken today.
static int window_steps = 0;
static Chain window_has_out(const Chain &c) {
    for (int k = 0; k < c.n; ++k)
        if (c.steps[k].kernel == Kernel::Window || c.steps[k].kernel == Kernel::WindowTeam) { ++window_steps; CHECK(c.steps[k].out >= 0 && c.steps[k].out < 4); }
    return c;
}
static Chain built(const LaunchPlan &plan, const Batch &b, Steering &st, ContextSteering &cs) { return window_has_out(build_chain(plan, b, st, cs)); }
static Chain tailed(const LaunchPlan &plan, const Chain &ran) { return window_has_out(tail_chain(plan, ran)); }

static bool step_is(const Step &s, Kernel k, int in, int out, int grid) { return s.kernel == k && s.in == in && s.out == out && s.grid == grid; }

static void test_plan() {
    const LaunchPlan p = plan_with(nullptr);
    // was kgpu_kernels.hip:681 ("40:4:32"), :700 (cus x per CU), :682 (no KGPU_POOL: auto)
    CHECK(p.n_pools == 1 && p.pool_bytes[0] == 40 * 1024 && p.pool_waves[0] == 4 && p.pool_max_pages[0] == 32 && p.pool_workgroups[0] == 1024);
    CHECK(p.pool_limit_auto);
    CHECK(p.alt_pool_bytes == 20 * 1024 && p.alt_pool_waves == 2 && p.alt_pool_workgroups == 2048);   // was :708-711
    CHECK(p.general_workgroups == 512);                                                                 // was :666
    CHECK(p.window_lds_bytes == 10 * 1024 && p.window_workgroups == 4096);                             // was :716-721
    CHECK(p.window_team_workgroups == 768 && p.window_team_mode == -1);                                 // was :724-726
    CHECK(p.window_first_bytes == 1024);                                                                 // was :728

    // two pools, default wavefronts 8 and pages 64 (was :684-694); an explicit KGPU_POOL turns the per-batch shape off (was :682, :710)
    const LaunchPlan q = plan_with("80:8,160:4");
    CHECK(q.n_pools == 2 && !q.pool_limit_auto && q.alt_pool_workgroups == 0);
    CHECK(q.pool_bytes[0] == 80 * 1024 && q.pool_waves[0] == 8 && q.pool_max_pages[0] == 64 && q.pool_workgroups[0] == 512);
    CHECK(q.pool_bytes[1] == 160 * 1024 && q.pool_waves[1] == 4 && q.pool_max_pages[1] == 64 && q.pool_workgroups[1] == 256);
    // out-of-range sizes and shapes without occupancy are left out; wavefronts cap at 16, pages at 64 (was :693-695)
    const LaunchPlan r = plan_with("4:4,40:4:99,200:4");
    CHECK(r.n_pools == 1 && r.pool_bytes[0] == 40 * 1024 && r.pool_max_pages[0] == 64);
    CHECK(plan_with("0").n_pools == 0);
    const LaunchPlan w = plan_with(nullptr, "0");   // no windowed kernel, so no team form either (was :717-724)
    CHECK(w.window_lds_bytes == 0 && w.window_workgroups == 0 && w.window_team_workgroups == 0);
    CHECK(plan_with(nullptr, nullptr, "2").window_team_mode == 2);
}

static void test_short_batch() {
    const LaunchPlan p = plan_with(nullptr);
    Steering st;
    ContextSteering cs;
    cs.win_share_q8 = 20;
    // pool -> window, no general while tail_batches is 0 (was kgpu_ctx.cpp:149, :153, :159; kgpu_kernels.hip:595)
    Chain c = built(p, batch(4096, 4096 * 40), st, cs);
    CHECK(c.n == 2 && c.event_behind_first && !c.small_scan && c.last_list() == 1);
    // pool grid: min(workgroups, ceil(n / waves)) (was kgpu_kernels.hip:563-565)
    CHECK(step_is(c.steps[0], Kernel::Pool, -1, 0, 1024) && c.steps[0].lds_bytes == 40 * 1024 && c.steps[0].waves == 4 && c.steps[0].max_pages == 32);
    // window grid: ((4096 * 20) >> 8) * 5 / 4 + 64 = 464 (was kgpu_ctx.cpp:190, kgpu_kernels.hip:540); expected (464 - 64) * 4 / 5 = 320 <= 464: no claim (was :543-544)
    CHECK(step_is(c.steps[1], Kernel::Window, 0, 1, 464) && !c.steps[1].claim && c.steps[1].lds_bytes == 10 * 1024);
    CHECK(step_is(built(p, batch(1000, 1000 * 40), st, cs).steps[0], Kernel::Pool, -1, 0, 250));
    // the context's first batch: the full grid (was kgpu_ctx.cpp:189)
    c = built(p, batch(4096, 4096 * 40, false), st, cs);
    CHECK(step_is(c.steps[1], Kernel::Window, 0, 1, 4096) && !c.steps[1].claim);
    // at least 256 (was kgpu_ctx.cpp:190)
    cs.win_share_q8 = 0;
    CHECK(built(p, batch(4096, 4096 * 40), st, cs).steps[1].grid == 256);
    // an estimate beyond the chip: the full grid, and the sentences are claimed one by one (was kgpu_kernels.hip:540-544)
    cs.win_share_q8 = 256;
    c = built(p, batch(65536, 65536 * 40), st, cs);
    CHECK(step_is(c.steps[1], Kernel::Window, 0, 1, 4096) && c.steps[1].claim);
    // disarmed windowed kernel: the pool alone (was kgpu_ctx.cpp:153-154)
    st.window_batches = 0;
    c = built(p, batch(4096, 4096 * 40), st, cs);
    CHECK(c.n == 1 && c.last_list() == 0);
    // armed general kernel: it closes the chain over the last list (was kgpu_ctx.cpp:159-160, kgpu_kernels.hip:547-551)
    st.window_batches = 64; st.tail_batches = 1;
    c = built(p, batch(4096, 4096 * 40), st, cs);
    CHECK(c.n == 3 && step_is(c.steps[2], Kernel::General, 1, -1, 512) && c.last_list() == -1);
    // two pools while big_pool_batches is armed (was kgpu_ctx.cpp:149, kgpu_kernels.hip:561-571)
    const LaunchPlan q = plan_with("80:8,160:4");
    st.tail_batches = 0; st.big_pool_batches = 1;
    c = built(q, batch(4096, 4096 * 40), st, cs);
    CHECK(c.n == 3 && step_is(c.steps[0], Kernel::Pool, -1, 0, 512) && step_is(c.steps[1], Kernel::Pool, 0, 1, 256) && c.steps[1].waves == 4);
    CHECK(c.steps[2].kernel == Kernel::Window && c.steps[2].in == 1 && c.steps[2].out == 2);
    st.big_pool_batches = 0;
    CHECK(built(q, batch(4096, 4096 * 40), st, cs).pools() == 1);
    // an empty batch has no chain (was kgpu_ctx.cpp:148)
    CHECK(built(p, batch(0, 0), st, cs).n == 0);
}

static void test_window_first() {
    const LaunchPlan p = plan_with(nullptr);
    // 1024 bytes per sentence on average or more (was kgpu_ctx.cpp:99)
    CHECK(starts_with_window(p, batch(1000, 1024000)) && !starts_with_window(p, batch(1000, 1023999)));
    CHECK(!starts_with_window(plan_with("0"), batch(1000, 3000000)) && !starts_with_window(plan_with(nullptr, "0"), batch(1000, 3000000)));
    {   // a lone batch: 1000 in flight <= 2 x 768 team workgroups -> the team form, the ordinary form behind it on a grid of 256 (was kgpu_ctx.cpp:166-172,
        // kgpu_kernels.hip:575-586)
        Steering st;
        ContextSteering cs;
        const Chain c = built(p, batch(1000, 3000000), st, cs);
        CHECK(c.n == 2 && !c.event_behind_first && c.small_scan && c.pools() == 0);
        CHECK(step_is(c.steps[0], Kernel::WindowTeam, -1, 0, 1000) && c.steps[0].lds_bytes == 10 * 1024);
        CHECK(step_is(c.steps[1], Kernel::Window, 0, 1, 256) && !c.steps[1].claim);   // expected (256 - 64) * 4 / 5 = 153
        CHECK(cs.counted_long == 1000 && st.long_sentences_in_flight == 1000 && st.long_peak == 1000);
        built(p, batch(1000, 3000000), st, cs);   // a rerun of the same batch counts it once (was kgpu_ctx.cpp:167)
        CHECK(cs.counted_long == 1000 && st.long_sentences_in_flight == 1000);
    }
    {   // other contexts' long sentences in flight: 2000 > 1536 -> the ordinary form over the identity, grid min(n, 4096) (was kgpu_kernels.hip:537)
        Steering st;
        ContextSteering cs;
        st.long_sentences_in_flight = 1000;
        const Chain c = built(p, batch(1000, 3000000), st, cs);
        CHECK(c.n == 1 && step_is(c.steps[0], Kernel::Window, -1, 0, 1000) && !c.steps[0].claim && c.small_scan && c.last_list() == 0);
    }
    {   // the peak decays by an eighth per enqueue (was kgpu_ctx.cpp:168-170): max(1000, 4000 - 500) = 3500
        Steering st;
        ContextSteering cs;
        st.long_peak = 4000;
        CHECK(built(p, batch(1000, 3000000), st, cs).steps[0].kernel == Kernel::Window && st.long_peak == 3500);
    }
    {   // boundary: a peak of exactly 2 x 768 still takes the team form
        Steering st;
        ContextSteering cs;
        st.long_sentences_in_flight = 536;
        CHECK(built(p, batch(1000, 3000000), st, cs).steps[0].kernel == Kernel::WindowTeam);
    }
    {   // more sentences than windowed workgroups: claimed one by one (was kgpu_kernels.hip:543-544)
        Steering st;
        ContextSteering cs;
        const Chain c = built(p, batch(5000, 6000000), st, cs);
        CHECK(step_is(c.steps[0], Kernel::Window, -1, 0, 4096) && c.steps[0].claim);
    }
    {   // KGPU_WINDOW_TEAM=0: never, and nothing is counted (was kgpu_ctx.cpp:166)
        Steering st;
        ContextSteering cs;
        const Chain c = built(plan_with(nullptr, nullptr, "0"), batch(1000, 3000000), st, cs);
        CHECK(c.n == 1 && c.steps[0].kernel == Kernel::Window && cs.counted_long == 0 && st.long_sentences_in_flight == 0);
    }
    {   // KGPU_WINDOW_TEAM=2: whatever the load (was kgpu_ctx.cpp:172)
        Steering st;
        ContextSteering cs;
        st.long_sentences_in_flight = 100000;
        CHECK(built(plan_with(nullptr, nullptr, "2"), batch(1000, 3000000), st, cs).steps[0].kernel == Kernel::WindowTeam);
    }
    {   // armed general kernel behind a team chain: over list 1 (was kgpu_kernels.hip:596)
        Steering st;
        ContextSteering cs;
        st.tail_batches = 64;
        const Chain c = built(p, batch(1000, 3000000), st, cs);
        CHECK(c.n == 3 && step_is(c.steps[2], Kernel::General, 1, -1, 512));
    }
    {   // no pools in the plan: every chain starts with the windowed kernel, the team rule applies (was kgpu_ctx.cpp:149, :166)
        Steering st;
        ContextSteering cs;
        const Chain c = built(plan_with("0"), batch(100, 1000), st, cs);
        CHECK(c.n == 2 && step_is(c.steps[0], Kernel::WindowTeam, -1, 0, 100));
    }
}

static void test_pool_shape() {
    const LaunchPlan p = plan_with(nullptr);
    Steering st;
    ContextSteering cs;
    cs.long_share = true;
    cs.win_share_q8 = 64;
    // long_share: two wavefronts on 20 KB, 56 pages up to 16 384 sentences, 64 beyond (was kgpu_ctx.cpp:181-184)
    Chain c = built(p, batch(16384, 16384 * 40), st, cs);
    CHECK(step_is(c.steps[0], Kernel::Pool, -1, 0, 2048) && c.steps[0].lds_bytes == 20 * 1024 && c.steps[0].waves == 2 && c.steps[0].max_pages == 56);
    CHECK(c.small_scan);   // a windowed launch in the chain and long_share (was kgpu_ctx.cpp:199)
    c = built(p, batch(16385, 16385 * 40), st, cs);
    CHECK(c.steps[0].max_pages == 64 && c.steps[0].lds_bytes == 20 * 1024);
    CHECK(built(p, batch(1000, 1000 * 40), st, cs).steps[0].grid == 500);   // ceil(1000 / 2)
    // an explicit KGPU_POOL keeps its shape (was kgpu_ctx.cpp:181)
    c = built(plan_with("40:4:32"), batch(16384, 16384 * 40), st, cs);
    CHECK(c.steps[0].lds_bytes == 40 * 1024 && c.steps[0].waves == 4 && c.steps[0].max_pages == 32);
    // "roomy": four reservations of ((bytes / n) * est >> 8) + 768 beyond 92 % of the pool -> three wavefronts, the same grid (was kgpu_ctx.cpp:104-105, :185)
    cs.long_share = false;
    Batch b = batch(4096, 4096 * 40);
    b.est_q8 = 55380;   // (40 * 55380 >> 8) + 768 = 9421; 400 * 9421 > 40960 * 92
    c = built(p, b, st, cs);
    CHECK(step_is(c.steps[0], Kernel::Pool, -1, 0, 1024) && c.steps[0].waves == 3 && c.steps[0].lds_bytes == 40 * 1024);
    b.n = 1000; b.bytes = 40000;
    CHECK(built(p, b, st, cs).steps[0].grid == 334);   // ceil(1000 / 3)
    b = batch(4096, 4096 * 40);
    b.est_q8 = 55379;   // 9420: fits
    CHECK(built(p, b, st, cs).steps[0].waves == 4);
    b.est_q8 = 65536;   // only the shipped plan (was kgpu_ctx.cpp:105)
    CHECK(built(plan_with("40:4"), b, st, cs).steps[0].waves == 4);
}

static void test_general_closes() {
    const LaunchPlan p = plan_with(nullptr);
    Steering st;
    ContextSteering cs;
    // ablation: the pool kernel and the general kernel, no windowed kernel, even for long sentences (was kgpu_ctx.cpp:99, :153, :159; kgpu_kernels.hip:573)
    Batch b = batch(1000, 3000000);
    b.stop_after = 3;
    Chain c = built(p, b, st, cs);
    // (3000 bytes per sentence: four reservations do not fit, so the pool runs three wavefronts: ceil(1000 / 3) workgroups)
    CHECK(c.n == 2 && step_is(c.steps[0], Kernel::Pool, -1, 0, 334) && c.steps[0].waves == 3 && step_is(c.steps[1], Kernel::General, 0, -1, 512) && !c.small_scan);
    b = batch(1, 100);   // lattice dump
    b.dump = true;
    c = built(p, b, st, cs);
    CHECK(c.n == 2 && step_is(c.steps[0], Kernel::Pool, -1, 0, 1) && step_is(c.steps[1], Kernel::General, 0, -1, 512));
    b = batch(1000, 3000000);   // the rerun without the windowed kernel: no window-first chain either
    b.no_window = true;
    c = built(p, b, st, cs);
    CHECK(c.n == 2 && c.steps[0].kernel == Kernel::Pool && step_is(c.steps[1], Kernel::General, 0, -1, 512) && cs.counted_long == 0);
    // nothing but the general kernel: over the identity, grid min(n, 512) (was kgpu_kernels.hip:550)
    c = built(plan_with("0", "0"), batch(100, 1000), st, cs);
    CHECK(c.n == 1 && step_is(c.steps[0], Kernel::General, -1, -1, 100) && !c.event_behind_first);
}

static void test_tail() {
    const LaunchPlan p = plan_with(nullptr), q = plan_with("80:8,160:4");
    Steering st;
    ContextSteering cs;
    cs.win_share_q8 = 20;
    // the windowed kernel was in the chain: the general kernel over its list (was kgpu_kernels.hip:604, :609)
    Chain t = tailed(p, built(p, batch(4096, 4096 * 40), st, cs));
    CHECK(t.n == 1 && step_is(t.steps[0], Kernel::General, 1, -1, 512) && !t.small_scan && !t.event_behind_first);
    // pool alone: the windowed kernel over list 0 on the full grid without claims, the general kernel over list 1 (was kgpu_kernels.hip:604-609)
    st.window_batches = 0;
    const Chain pool_only = built(p, batch(4096, 4096 * 40), st, cs);
    t = tailed(p, pool_only);
    CHECK(t.n == 2 && step_is(t.steps[0], Kernel::Window, 0, 1, 4096) && !t.steps[0].claim && step_is(t.steps[1], Kernel::General, 1, -1, 512));
    // two pools alone (list 1) and with the windowed kernel (list 2)
    st.big_pool_batches = 1;
    t = tailed(q, built(q, batch(4096, 4096 * 40), st, cs));
    CHECK(t.n == 2 && step_is(t.steps[0], Kernel::Window, 1, 2, 4096) && step_is(t.steps[1], Kernel::General, 2, -1, 512));
    st.window_batches = 64;
    t = tailed(q, built(q, batch(4096, 4096 * 40), st, cs));
    CHECK(t.n == 1 && step_is(t.steps[0], Kernel::General, 2, -1, 512));
    // window-first chains: after the team form (list 1) and without it (list 0)
    Steering st2;
    ContextSteering cs2;
    t = tailed(p, built(p, batch(1000, 3000000), st2, cs2));
    CHECK(t.n == 1 && step_is(t.steps[0], Kernel::General, 1, -1, 512));
    t = tailed(p, built(plan_with(nullptr, nullptr, "0"), batch(1000, 3000000), st2, cs2));
    CHECK(t.n == 1 && step_is(t.steps[0], Kernel::General, 0, -1, 512));
    // no windowed kernel in the plan: the general kernel over the pool's list
    t = tailed(plan_with(nullptr, "0"), pool_only);
    CHECK(t.n == 1 && step_is(t.steps[0], Kernel::General, 0, -1, 512));
}

static Control counts(unsigned o0, unsigned o1 = 0, unsigned o2 = 0, unsigned late0 = 0) {
    Control h;
    memset(&h, 0, sizeof h);
    h.ovf_count[0] = o0; h.ovf_count[1] = o1; h.ovf_count[2] = o2; h.late_count[0] = late0;
    return h;
}

static void test_feedback() {
    const LaunchPlan p = plan_with(nullptr);
    const uint32_t E = 64 * 256;
    ContextSteering cs;
    cs.win_share_q8 = 20;
    Steering st;
    st.tail_batches = 64;
    const Chain full = built(p, batch(1000, 40000), st, cs);   // pool -> window -> general
    st.tail_batches = 0;
    const Chain pw = built(p, batch(1000, 40000), st, cs);     // pool -> window
    st.window_batches = 0;
    const Chain po = built(p, batch(1000, 40000), st, cs);     // pool
    CHECK(full.n == 3 && pw.n == 2 && po.n == 1);
    const uint32_t late_ok = 20;   // 2 %: the estimate stays

    // arming of the windowed kernel: what the pools left sets 64, a clean batch with it in the chain takes 8 (was kgpu_ctx.cpp:374-375)
    st.window_batches = 10; st.tail_batches = 10; st.est_q8 = E;
    chain_feedback(p, pw, nullptr, counts(5, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.window_batches == 64 && st.tail_batches == 10);   // the window left nothing, the general kernel was not in the chain: unchanged
    chain_feedback(p, pw, nullptr, counts(0, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.window_batches == 56);
    st.window_batches = 10;
    chain_feedback(p, po, nullptr, counts(0, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.window_batches == 10 && st.tail_batches == 10);   // the windowed kernel was not in the chain: no decay, and the general kernel is not armed from the pools (was :377)
    // arming of the general kernel from the windowed kernel's list (was kgpu_ctx.cpp:378-380)
    chain_feedback(p, pw, nullptr, counts(5, 1, 0, late_ok), 1000, E, st, cs);
    CHECK(st.tail_batches == 64);
    chain_feedback(p, full, nullptr, counts(5, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.tail_batches == 56);
    // a tail pass that added the windowed kernel: its list arms the general kernel, the first pass's chain decides the decay (was kgpu_ctx.cpp:263, :355-358, :377-380)
    const Chain tail = tailed(p, po);
    st.window_batches = 10; st.tail_batches = 10;
    chain_feedback(p, po, &tail, counts(3, 1, 0, late_ok), 1000, E, st, cs);
    CHECK(st.window_batches == 64 && st.tail_batches == 64);
    chain_feedback(p, po, &tail, counts(3, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.tail_batches == 64);   // the first pass had no general kernel: no decay
    // without a windowed kernel in the plan the pools' list arms the general kernel (was kgpu_ctx.cpp:377-378)
    const LaunchPlan nw = plan_with(nullptr, "0");
    st.tail_batches = 10;
    chain_feedback(nw, po, nullptr, counts(2, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(st.tail_batches == 64 && cs.win_share_q8 == 0);   // (and no share: was kgpu_ctx.cpp:384)

    // long_share: entered at 32 / 256, left below 16 (was kgpu_ctx.cpp:384-385)
    cs = ContextSteering{};
    chain_feedback(p, pw, nullptr, counts(124, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(cs.win_share_q8 == 31 && !cs.long_share);
    chain_feedback(p, pw, nullptr, counts(125, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(cs.win_share_q8 == 32 && cs.long_share);
    chain_feedback(p, pw, nullptr, counts(63, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(cs.win_share_q8 == 16 && cs.long_share);
    chain_feedback(p, pw, nullptr, counts(62, 0, 0, late_ok), 1000, E, st, cs);
    CHECK(cs.win_share_q8 == 15 && !cs.long_share);
    chain_feedback(p, pw, nullptr, counts(1000, 0, 0, late_ok), 10, E, st, cs);
    CHECK(cs.win_share_q8 == 256);   // clamped

    // est_q8 steering on the late count of the first pool (was kgpu_ctx.cpp:401-407): +1/4 above a quarter, +1/16 above 1/32, -1/128 below 1 %
    auto est_after = [&](unsigned late, uint32_t est) {
        st.est_q8 = 7;   // (a value no branch produces: stays when the estimate does not change)
        chain_feedback(p, pw, nullptr, counts(0, 0, 0, late), 1000, est, st, cs);
        return (uint32_t)st.est_q8;
    };
    CHECK(est_after(251, E) == E + E / 4);
    CHECK(est_after(250, E) == E + E / 16);
    CHECK(est_after(32, E) == E + E / 16);
    CHECK(est_after(31, E) == 7);
    CHECK(est_after(10, E) == 7);
    CHECK(est_after(9, E) == E - E / 128);
    CHECK(est_after(0, 16 * 256) == 7);                 // clamped at 16 x 256: no change, no store
    CHECK(est_after(0, 16 * 256 + 4) == 16 * 256);
    CHECK(est_after(500, 1024 * 256) == 7);             // ... and at 1024 x 256
    CHECK(est_after(500, 1000 * 256) == 1024 * 256);

    // big_pool_batches with two pools: what the first pool left sets 64, a clean two-pool batch takes 1 (was kgpu_ctx.cpp:397-400)
    const LaunchPlan q = plan_with("80:8,160:4");
    Steering s2;
    ContextSteering c2;
    const Chain one = built(q, batch(1000, 40000), s2, c2);
    s2.big_pool_batches = 1;
    const Chain two = built(q, batch(1000, 40000), s2, c2);
    CHECK(one.pools() == 1 && two.pools() == 2);
    s2.big_pool_batches = 5;
    chain_feedback(q, two, nullptr, counts(0, 0, 0, late_ok), 1000, E, s2, c2);
    CHECK(s2.big_pool_batches == 4);
    chain_feedback(q, one, nullptr, counts(0, 0, 0, late_ok), 1000, E, s2, c2);
    CHECK(s2.big_pool_batches == 4);
    chain_feedback(q, one, nullptr, counts(1, 0, 0, late_ok), 1000, E, s2, c2);
    CHECK(s2.big_pool_batches == 64);
    // ... the windowed kernel is armed by the LAST pool's list (was kgpu_ctx.cpp:372)
    s2.window_batches = 10;
    chain_feedback(q, two, nullptr, counts(3, 0, 0, late_ok), 1000, E, s2, c2);
    CHECK(s2.window_batches == 2);   // list 1 empty, the windowed kernel in the chain: -8
    chain_feedback(q, two, nullptr, counts(0, 3, 0, late_ok), 1000, E, s2, c2);
    CHECK(s2.window_batches == 64 && c2.win_share_q8 == 0);   // (3 * 256 / 1000 = 0)

    // a window-first chain: the windowed kernel's list arms the general kernel, 1 after the team form, 0 without (was kgpu_ctx.cpp:387-391)
    Steering s3;
    ContextSteering c3;
    const Chain team = built(p, batch(1000, 3000000), s3, c3);
    CHECK(team.steps[0].kernel == Kernel::WindowTeam);
    s3.tail_batches = 10; s3.window_batches = 10; s3.est_q8 = 7;
    chain_feedback(p, team, nullptr, counts(5, 0, 0, 900), 1000, E, s3, c3);
    CHECK(s3.tail_batches == 10 && s3.window_batches == 10 && s3.est_q8 == 7 && c3.win_share_q8 == 0);   // no pools: no window arming, no share, no estimate
    chain_feedback(p, team, nullptr, counts(0, 1), 1000, E, s3, c3);
    CHECK(s3.tail_batches == 64);
    const Chain lone = built(plan_with(nullptr, nullptr, "0"), batch(1000, 3000000), s3, c3);
    s3.tail_batches = 10;
    chain_feedback(p, lone, nullptr, counts(1), 1000, E, s3, c3);
    CHECK(s3.tail_batches == 64);
    s3.tail_batches = 64;
    const Chain lone_general = built(plan_with(nullptr, nullptr, "0"), batch(1000, 3000000), s3, c3);
    chain_feedback(p, lone_general, nullptr, counts(0), 1000, E, s3, c3);
    CHECK(lone_general.n == 2 && s3.tail_batches == 56);
    // ... not without pools in the plan (was kgpu_ctx.cpp:387: plan.n_pools)
    s3.tail_batches = 10;
    chain_feedback(plan_with("0"), built(plan_with("0"), batch(100, 1000), s3, c3), nullptr, counts(1, 1), 100, E, s3, c3);
    CHECK(s3.tail_batches == 10);

    // an empty batch changes nothing
    st.window_batches = 10; st.tail_batches = 10; st.est_q8 = 7;
    chain_feedback(p, built(p, batch(0, 0), st, cs), nullptr, counts(0), 0, E, st, cs);
    CHECK(st.window_batches == 10 && st.tail_batches == 10 && st.est_q8 == 7);
}

int main() {
    test_plan();
    test_short_batch();
    test_window_first();
    test_pool_shape();
    test_general_closes();
    test_tail();
    test_feedback();
    CHECK(window_steps >= 30);   // (the wrappers above saw the chains)
    if (failures) { printf("%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d checks\n", checks);
    return 0;
}
