// kanpyo_amd/csrc/kgpu_chain.h -- the launch-chain policy: which kernels a batch gets, in what order, over which work lists, and how the
// outcome steers the next batch.  Plain host C++ (no HIP header): tests/c_abi/chain_policy.cpp builds kgpu_chain.cpp with g++ alone.
// kgpu_ctx.cpp runs a chain step by step (kgpu_kernels.hip: launch_step); this file is the only place that knows the work-list indices.
#pragma once
#include <atomic>
#include <cstdint>

#include "kgpu_internal.h"

namespace kgpu {

// Launch plan of a context: the LDS page-pool kernel (kgpu_pool.hip) once or twice -- W independent wavefronts per workgroup share pool_bytes of
// LDS, each sentence takes what it needs -- then the windowed kernel (kgpu_window.hip: bounded LDS whatever the length) for whatever fits no
// pool, then the general kernel, whose lattices live in HBM scratch, as the last resort.  A sentence that a launch cannot serve is pushed onto
// the next launch's work list.
struct LaunchPlan {
    int n_pools;
    uint32_t pool_bytes[2];
    uint32_t pool_waves[2];
    uint32_t pool_max_pages[2];  // of 64: larger reservations are routed to the next launch
    bool pool_limit_auto;        // the shipped plan (no KGPU_POOL): the chain may pick the pool shape per batch (build_chain)
    uint32_t alt_pool_bytes, alt_pool_waves;   // ... the shape for chains that hold a windowed launch: smaller workgroups (20 KB, two wavefronts) find their LDS
    int alt_pool_workgroups;                   // sooner on a chip full of 10 KB single-wavefront workgroups (0: not available)
    int pool_workgroups[2];   // persistent grid per pool launch
    int general_workgroups;
    uint32_t window_lds_bytes;  // > 0: the windowed kernel (kgpu_window.hip) behind the pools; 0: the general kernel serves what they route away
    int window_workgroups;
    int window_team_workgroups;  // resident workgroups of its two-wavefronts-per-sentence form on the whole chip (0: not available)
    int window_team_mode;        // KGPU_WINDOW_TEAM: 0 never, 2 whenever the chain starts with the windowed kernel, -1 (default) by the load
    uint32_t window_first_bytes; // KGPU_WINDOW_FIRST: a batch averaging this many bytes per sentence or more gets no pool launch in front (default 1024; 0 = never)
};

// Resident workgroups per CU of each kernel shape (kgpu_pool.hip, kgpu_window.hip; a test passes fixed values).
struct Occupancy {
    int (*pool)(uint32_t pool_bytes, uint32_t waves);
    int (*window)(uint32_t lds_bytes);
    int (*window_team)(uint32_t lds_bytes);
};
LaunchPlan make_launch_plan(int compute_units, const Occupancy &occ);   // reads KGPU_POOL, KGPU_WINDOW, KGPU_WINDOW_TEAM, KGPU_WINDOW_FIRST

// One launch of a chain.  Work lists are BatchArgs::ovf[k] with their lengths in Control::ovf_count[k]; a pool launch also counts its late
// deferrals in Control::late_count[out].
enum class Kernel : uint8_t { Pool, WindowTeam, Window, General };
struct Step {
    Kernel kernel;
    int in;              // work list read (-1: the identity over [0, n))
    int out;             // work list written (-1: none, the general kernel)
    int grid;            // workgroups
    uint32_t lds_bytes;  // Pool: the pool's LDS; Window / WindowTeam: each wavefront's
    uint32_t waves;      // wavefronts per workgroup (the windowed kernel: 1, its team form 2)
    uint32_t max_pages;  // Pool: larger reservations go on to the next launch
    bool claim;          // Window: its workgroups claim sentences one by one instead of every grid-th being theirs
};

struct Chain {
    Step steps[4];                    // at most two pools or the team form, the windowed kernel, the general kernel
    int n = 0;
    bool event_behind_first = false;  // the first-launch event goes behind steps[0] (a pool launch); otherwise in front of the chain
    bool small_scan = false;          // the scan / compaction behind it runs small workgroups (launch_scan_compact)
    bool aux_one_launch = false;      // ... is ONE launch without LDS (k_aux_one_launch): a pool launch in front, no small_scan, at most AUX_ONE_LAUNCH_MAX sentences
    int pools() const;
    const Step *find(Kernel k) const;
    int last_list() const { return n ? steps[n - 1].out : -1; }   // >= 0: the chain ended without the general kernel, on this list
};

// The largest batch whose scan and compaction are one launch: every wavefront of that launch sums the counts in front of its sentences itself, reads that
// grow with the square of the batch (measured at 4096; larger batches keep the two launches).
constexpr uint64_t AUX_ONE_LAUNCH_MAX = 4096;

// What the chain of a batch is built from.
struct Batch {
    uint64_t n, bytes;
    uint32_t est_q8;       // BatchArgs::est_q8
    uint32_t stop_after;   // kgpu_ctx_set_ablation
    bool dump;             // kgpu_lattice_dump
    bool no_window;        // a rerun without the windowed kernel (it had flagged Control::window_fail)
    bool share_known;      // the context has a batch behind it since its routing counters were reset (its win_share_q8 is an estimate)
};

// The dictionary-wide state that steers the chain, shared by its contexts (relaxed atomics: a race only loses an adjustment).
struct Steering {
    // LDS bytes reserved per input byte (x256) by the pool kernel before the lattice is known; a property of the dictionary + the text
    std::atomic<uint32_t> est_q8{64 * 256};   // (round 6: the lattice takes ~52 bytes of LDS per input byte on IPADIC-shaped text; was 80)
    // Batches left for which the second (whole-CU) pool is launched.  Its workgroups need a CU's entire LDS just to start and find their list empty,
    // which stalls them -- and the launches queued behind -- until both 80 KB pools of that CU have drained; so it is only issued while recent batches
    // actually overflowed the first pool.  Performance heuristic only: the chain is complete either way.
    std::atomic<int> big_pool_batches{0};
    std::atomic<int> window_batches{64};  // the windowed kernel: in the chain while recent batches left the pools sentences (starts armed)
    std::atomic<int> tail_batches{0};     // the general kernel behind it: while recent batches left the windowed kernel (or, without one, the pools) sentences
    std::atomic<int> long_sentences_in_flight{0};   // sentences of window-first batches between enqueue and completion (decides the two-wavefront form)
    std::atomic<int> long_peak{0};                  // ... its recent maximum (decays by an eighth per enqueue): a caller that keeps eight batches in flight is not
                                                    // mistaken for a lone one by the batch that happens to be enqueued while the others are being collected
};
// ... and a context's own.
struct ContextSteering {
    uint32_t win_share_q8 = 0;  // share of the last pool-first batch's sentences that the pools routed to the windowed kernel (x256)
    bool long_share = false;    // ... an eighth or more, with hysteresis (left below a sixteenth): the context runs its batches on a long stream
    int counted_long = 0;       // what the pending batch added to Steering::long_sentences_in_flight (the context returns it when the batch is over)
};

bool starts_with_window(const LaunchPlan &plan, const Batch &b);   // the chain has no pool launch in front of the windowed kernel
Chain build_chain(const LaunchPlan &plan, const Batch &b, Steering &st, ContextSteering &cs);
Chain tail_chain(const LaunchPlan &plan, const Chain &ran);   // what a chain that ended on a work list left out, over that list
// The outcome of a batch: `ran` is its (first) chain, `tail` the tail pass behind it or nullptr, `h` the published control block (after a tail
// pass: the first pass's lists up to the one the tail served), est_q8 the estimate the batch ran with.
void chain_feedback(const LaunchPlan &plan, const Chain &ran, const Chain *tail, const Control &h, uint64_t n, uint32_t est_q8, Steering &st,
                    ContextSteering &cs);

// Which of a dictionary's shared streams a batch goes to: the one with the least load, where a stream's load is the weight of the batches the host
// knows to be in flight on it (added at the enqueue, taken off when the batch's context retires it).  A weight is the batch's bytes -- a tail batch of
// 1696 sentences weighs what it costs, not what a full one does -- and a constant, so that empty batches count.  Eight contexts handed round-robin
// to three streams load them 3 : 3 : 2 for good, and the job then runs at the pace of the streams that carry three.
constexpr uint64_t STREAM_BATCH_BASE = 256;
inline uint64_t stream_batch_weight(uint64_t total_bytes) { return total_bytes + STREAM_BATCH_BASE; }
// -> the least-loaded of load[0 .. n); ties go to the first candidate at or after the cursor, which moves past the pick (equal loads: strict rotation).
// Loads within an eighth of each other tie: the chunks of a large host call differ by a few per cent in bytes, and the host retires them in order while
// the streams drain independently -- told apart byte by byte, streams that hold three such chunks each are picked at random, one ends up with four while
// another runs dry, and the call loses a sixth of its rate against plain rotation (profiles/experiments/stream_balance.txt).  A stream with a batch fewer
// among up to seven, or with a tail batch in a full one's place, is outside the band.
constexpr uint64_t STREAM_TIE_SHARE = 8;
// Relaxed atomics, as Steering: two callers that pick the same stream at once lose nothing but a little balance.
unsigned pick_stream(const std::atomic<uint64_t> *load, unsigned n, std::atomic<unsigned> &cursor);

}  // namespace kgpu
