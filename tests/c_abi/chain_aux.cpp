// Chain::aux_one_launch (kanpyo_amd/csrc/kgpu_chain.cpp: build_chain) on the CPU, no device: which batches get their scan and compaction as ONE
// launch without LDS.  tests/test_chain_aux_cpu.py builds this file with g++ against kgpu_chain.cpp alone.  Prints "ok <checks>" or FAIL lines.
#include <cstdio>
#include <cstdlib>

#include "../../kanpyo_amd/csrc/kgpu_chain.h"

using namespace kgpu;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) { ++failures; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// fake occupancies (as in chain_policy.cpp): 40 KB x 4 -> 4 per CU, 20 KB x 2 -> 8; windowed 10 KB -> 16, its team form -> 3
static int pool_occ(uint32_t bytes, uint32_t waves) { return bytes == 40 * 1024 && waves == 4 ? 4 : bytes == 20 * 1024 && waves == 2 ? 8 : 0; }
static int window_occ(uint32_t bytes) { return bytes == 10 * 1024 ? 16 : 0; }
static int team_occ(uint32_t bytes) { return bytes == 10 * 1024 ? 3 : 0; }

static LaunchPlan plan_with(const char *pool, const char *window) {
    pool ? setenv("KGPU_POOL", pool, 1) : unsetenv("KGPU_POOL");
    window ? setenv("KGPU_WINDOW", window, 1) : unsetenv("KGPU_WINDOW");
    unsetenv("KGPU_WINDOW_TEAM");
    unsetenv("KGPU_WINDOW_FIRST");
    return make_launch_plan(256, Occupancy{pool_occ, window_occ, team_occ});
}
static Batch batch(uint64_t n, uint64_t bytes_each) { return Batch{n, n * bytes_each, 64 * 256, 0, false, false, true}; }

int main() {
    const LaunchPlan p = plan_with(nullptr, nullptr);
    const uint64_t L = AUX_ONE_LAUNCH_MAX;
    CHECK(L >= 4096);   // a batch of 4096 is below the limit in any case
    CHECK(!Chain{}.aux_one_launch);   // the default is the old behaviour: what tail_chain returns, and an empty batch's chain
    {   // pool-only chains (the windowed kernel disarmed): on both sides of the limit
        Steering st;
        ContextSteering cs;
        st.window_batches = 0;
        for (uint64_t n : {uint64_t(1), uint64_t(3), uint64_t(4), uint64_t(5), uint64_t(255), uint64_t(4095), uint64_t(4096), L}) {
            const Chain c = build_chain(p, batch(n, 40), st, cs);
            CHECK(c.n == 1 && c.pools() == 1 && !c.small_scan && c.aux_one_launch);
        }
        for (uint64_t n : {L + 1, 2 * L, uint64_t(65536), uint64_t(1) << 20}) {
            const Chain c = build_chain(p, batch(n, 40), st, cs);
            CHECK(c.n == 1 && c.pools() == 1 && !c.small_scan && !c.aux_one_launch);
        }
        const Chain e = build_chain(p, batch(0, 0), st, cs);
        CHECK(e.n == 0 && !e.aux_one_launch);
    }
    {   // the pool with the windowed kernel armed behind it, the context's share of routed sentences small: small_scan is off, so it is one launch
        Steering st;
        ContextSteering cs;
        cs.win_share_q8 = 4;
        Chain c = build_chain(p, batch(4096, 40), st, cs);
        CHECK(c.n == 2 && c.find(Kernel::Window) && !c.small_scan && c.aux_one_launch);
        c = build_chain(p, batch(L + 1, 40), st, cs);
        CHECK(c.n == 2 && !c.small_scan && !c.aux_one_launch);
        // ... and with the general kernel armed behind both
        st.tail_batches = 1;
        c = build_chain(p, batch(4096, 40), st, cs);
        CHECK(c.n == 3 && c.find(Kernel::General) && !c.small_scan && c.aux_one_launch);
    }
    {   // long_share: the context's chains hold long windowed launches -- small_scan, two launches of small workgroups, whatever the batch size
        Steering st;
        ContextSteering cs;
        cs.win_share_q8 = 64; cs.long_share = true;
        for (uint64_t n : {uint64_t(1), uint64_t(4096), L, L + 1}) {
            const Chain c = build_chain(p, batch(n, 40), st, cs);
            CHECK(c.pools() == 1 && c.find(Kernel::Window) && c.small_scan && !c.aux_one_launch);
        }
        // ... unless the windowed kernel is not in the chain
        st.window_batches = 0;
        const Chain c = build_chain(p, batch(4096, 40), st, cs);
        CHECK(c.n == 1 && !c.small_scan && c.aux_one_launch);
    }
    {   // windowed chains: no pool launch in front (long sentences), or no pool kernel at all
        Steering st;
        ContextSteering cs;
        Chain c = build_chain(p, batch(1000, 3000), st, cs);
        CHECK(c.pools() == 0 && c.small_scan && !c.aux_one_launch);
        st.long_sentences_in_flight = 100000;   // the ordinary form
        c = build_chain(p, batch(1000, 3000), st, cs);
        CHECK(c.n == 1 && c.steps[0].kernel == Kernel::Window && c.small_scan && !c.aux_one_launch);
        const LaunchPlan w = plan_with("0", nullptr);
        ContextSteering cw;
        c = build_chain(w, batch(4096, 40), st, cw);
        CHECK(c.pools() == 0 && c.small_scan && !c.aux_one_launch);
        const LaunchPlan g = plan_with("0", "0");   // the general kernel alone
        c = build_chain(g, batch(4096, 40), st, cw);
        CHECK(c.n == 1 && c.steps[0].kernel == Kernel::General && !c.small_scan && !c.aux_one_launch);
    }
    {   // tail chains: over a work list, behind a first pass that has published its control block -- the old two launches
        Steering st;
        ContextSteering cs;
        st.window_batches = 0;
        const Chain ran = build_chain(p, batch(4096, 40), st, cs);
        CHECK(ran.aux_one_launch && ran.last_list() == 0);
        const Chain t = tail_chain(p, ran);
        CHECK(t.n == 2 && !t.small_scan && !t.aux_one_launch);
        const LaunchPlan nw = plan_with(nullptr, "0");
        const Chain ran2 = build_chain(nw, batch(4096, 40), st, cs);
        CHECK(ran2.n == 1 && ran2.aux_one_launch);
        const Chain t2 = tail_chain(nw, ran2);
        CHECK(t2.n == 1 && t2.steps[0].kernel == Kernel::General && !t2.aux_one_launch);
    }
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
