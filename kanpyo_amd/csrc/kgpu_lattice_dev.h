// kanpyo_amd/csrc/kgpu_lattice_dev.h -- one view of a kept lattice for the kernels that decode over it (kgpu_graphviz.hip, kgpu_nbest.hip, kgpu_prob.hip,
// kgpu_mode.hip, kgpu_user.hip; DESIGN.md, "The kept-lattice protocol"): the descriptor k_tokenize_general leaves per sentence under BatchArgs::keep_lattice (the LAT_*
// words of kgpu_internal.h), the two slabs it points to, the slab a forward kernel takes behind them, and the record of a node.  The layout of the slabs is
// written HERE and nowhere else.
//
// LAT_OWN is the consumer's own word: graphviz keeps the sentence's visible nodes there; the forward kernels of the other four keep the arena offset of
// their slab (lists; alpha | beta | best, or alpha | picks; state | kanji counts; a head with the user nodes' number, the user nodes, state | kanji counts and the
// user nodes by start and by end), and each file has a small struct of its own for what lies there.
#pragma once
#include "kgpu_device.h"
#include "kgpu_nbest_core.h"

namespace kgpu {
namespace dev {

struct KeptLat {
    bool valid;                    // false: nothing else is set
    uint32_t B, C, N;              // the sentence's bytes, characters, nodes (BOS is node 0, EOS node N - 1; nodes are numbered by start position)
    int32_t eos_dp;                // dp of EOS as tokenize found it
    uint64_t own;                  // LAT_OWN
    // slab A: u32[B + 4] arrays
    const uint32_t *cbyte;         // [C + 1]: a character position's byte offset
    const uint32_t *nb, *boff;     // [C + 2] each: the nodes that START at q are [nb[q], nb[q + 1]); the bucket slots of the nodes that END at q are [boff[q], boff[q + 1])
    uint32_t *path;                // the backtrace array, dead behind the tokenize kernel: u32 per position, a consumer's to use
    // slab N
    const uint4 *nodeA;            // [N]: x = left id | right id << 16, y = word cost, z = the node's bucket slot, w = sid (> 0 known, < 0 unknown, 0 BOS / EOS)
    const uint4 *bucket;           // [N] slots: x = the ending node's dp, y = its right id, z = its index
    const uint2 *nodeB;            // [N]: x, y = start and end character position
    const uint32_t *pre;           // [N]: tokenize's best predecessor
    uint8_t *scratch;              // lat_scratch_bytes(N) behind them (kgpu_internal.h: graphviz's arrays)
};

// Sentence s's view.  UNIFORM: every lane of the caller asks for the same s (a workgroup per sentence), and valid, B, C and N come back as wave-uniform
// values (scalar registers: loop bounds and branches around barriers); the slab offsets stay per-lane values, as the sweeps were measured.
template <bool UNIFORM = false>
__device__ __forceinline__ KeptLat kept_lat(uint8_t *arena, const unsigned long long *desc, uint64_t s) {
    KeptLat l{};
    const unsigned long long *ds = desc + LAT_DESC_WORDS * s;
    const uint32_t valid = (uint32_t)ds[LAT_VALID];
    l.valid = (UNIFORM ? bcast32(valid) : valid) != 0;
    if (!l.valid) return l;
    l.B = (uint32_t)ds[LAT_B]; l.C = (uint32_t)ds[LAT_C]; l.N = (uint32_t)ds[LAT_N];
    if (UNIFORM) { l.B = bcast32(l.B); l.C = bcast32(l.C); l.N = bcast32(l.N); }
    l.eos_dp = (int32_t)(uint32_t)ds[LAT_EOS_DP];
    l.own = ds[LAT_OWN];
    uint32_t *sa = (uint32_t *)(arena + ds[LAT_SLAB_A]);
    const uint64_t na = (uint64_t)l.B + 4, N = l.N;
    l.cbyte = sa + SLAB_A_CBYTE * na; l.nb = sa + SLAB_A_NB * na; l.boff = sa + SLAB_A_BOFF * na; l.path = sa + SLAB_A_PATH * na;
    uint8_t *sn = arena + ds[LAT_SLAB_N];
    l.nodeA = (const uint4 *)sn; l.bucket = (const uint4 *)(sn + N * 16); l.nodeB = (const uint2 *)(sn + N * 32); l.pre = (const uint32_t *)(sn + N * 40);
    l.scratch = sn + lat_scratch_off(N);
    return l;
}

// The forward kernels' slab: `bytes` of arena behind the lattices for the workgroup's sentence (descriptor ds, N nodes), taken by wavefront 0 and told to
// the other wavefronts through *lds_off -> its arena offset, stored in ds[LAT_OWN]; or LAT_NO_SLAB -- the arena is full (Control::arena_overflow is then
// set: the host's retry) or N >= node_cap -- and the sentence has KGPU_SENT_NO_SCRATCH in *status and its valid word cleared: no later launch looks at it.
// Called by ALL threads of the workgroup from workgroup-uniform control flow: two barriers inside, and the caller's branch on the result is workgroup-
// uniform as well (it tests what came through *lds_off; the descriptor is written by this workgroup alone).
constexpr uint64_t LAT_NO_SLAB = ~0ull;
__device__ __forceinline__ BatchArgs lat_arena_args(Control *ctl, uint8_t *arena, uint64_t arena_bytes) {   // (what slab_fresh reads)
    BatchArgs a{};
    a.ctl = ctl; a.arena = arena; a.arena_bytes = arena_bytes;
    return a;
}
__device__ __forceinline__ uint64_t lat_take_slab(unsigned long long *ds, uint64_t bytes, uint64_t N, uint64_t node_cap, unsigned long long *lds_off,
                                                  const BatchArgs &arena, uint8_t *status) {
    const uint32_t lane = threadIdx.x & 63u;
    if (bcast32(threadIdx.x >> 6) == 0) {
        Slab sl{nullptr, 0};
        const bool ok = N < node_cap && slab_fresh(sl, bytes, arena, lane);
        if (lane == 0) *lds_off = ok ? (unsigned long long)(sl.ptr - arena.arena) : LAT_NO_SLAB;
    }
    __syncthreads();
    const uint64_t off = bcast64(*lds_off);
    __syncthreads();   // (read by all before the next sentence's is stored)
    if (threadIdx.x == 0) {
        if (off == LAT_NO_SLAB) { *status = KGPU_SENT_NO_SCRATCH; ds[LAT_VALID] = 0; }
        else ds[LAT_OWN] = off;
    }
    return off;
}

__device__ __forceinline__ uint32_t class_of(int32_t sid) { return sid > 0 ? KGPU_CLASS_KNOWN : sid < 0 ? KGPU_CLASS_UNKNOWN : KGPU_CLASS_DUMMY; }
// The 24-byte record of node t, as tokenize writes a token's.
__device__ __forceinline__ kgpu_token lat_record(const KeptLat &l, uint32_t t) {
    const int32_t sid = (int32_t)l.nodeA[t].w;
    const uint2 se = l.nodeB[t];
    const uint32_t bs = l.cbyte[se.x];
    return nbest_record(class_of(sid), sid < 0 ? -sid : sid, bs, se.x, se.y, l.cbyte[se.y] - bs);
}

}  // namespace dev
}  // namespace kgpu
