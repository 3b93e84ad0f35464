// kanpyo_amd/csrc/kgpu_backtrace_core.h -- the pool kernel's backtrace over QUADS (kgpu_pool.hip, phase 5; lattice.rs:144-153): the rules by which a node's
// best predecessor is doubled into its four nearest ancestors, and by which the chase over those quads ends.  No HIP in here: the kernel's passes go through
// these functions, and tests/c_abi/backtrace_core.cpp runs the same functions on the host against the plain one-step chase (tests/test_backtrace_core_cpu.py).
//
// A node is 8 bytes {x, y}.  Behind stage B only the LOW HALF of y is alive: pre[t], the best predecessor, BT_NONE where there is none (BOS, a dead node, a
// live node nothing reached).  The other three half-words are overlaid:
//   level 1   y = p1 | p2 << 16          p2[t] = p1[p1[t]]
//   level 2   x = p3 | p4 << 16          p3[t] = p1[p2[t]], p4[t] = p2[p2[t]]: the WHOLE y word of node p2[t]
// BT_NONE propagates -- a node whose k-th ancestor does not exist has BT_NONE there -- without a select on the value and without a read at index 0xFFFF: a
// hop from BT_NONE reads entry N, one behind the last node (node indices are below N <= 0xFFFF, so that is min(p, N)), which the kernel has made all BT_NONE
// before level 1.  (Indices fall strictly along a chain, so every chain ends.)
#pragma once
#include <cstdint>

#include "kgpu_tilepack.h"   // KGPU_HD

namespace kgpu {

constexpr uint32_t BT_NONE = 0xFFFFu;
constexpr uint32_t BT_QUAD = 4;   // path entries a round of the chase may write: pos, p1, p2, p3 (it goes on from p4)

// the entry a hop from p reads: node p, or entry N -- all BT_NONE -- for "no such ancestor".  N: the sentence's nodes, BOS and EOS included, 2 <= N <= 0xFFFF
KGPU_HD constexpr uint32_t bt_hop(uint32_t p, uint32_t N) { return p < N ? p : N; }
// level 1, node t: p2[t] = the half-word p1 of entry bt_hop(p1[t]), stored into the upper half of y by a half-word store (other lanes read the lower half of
// the same word in the same pass).  Level 2, after level 1 of EVERY node: x of node t = the y word of entry bt_hop(p2[t]).
KGPU_HD constexpr uint32_t bt_p1(uint32_t y) { return y & 0xFFFFu; }
KGPU_HD constexpr uint32_t bt_p2(uint32_t y) { return y >> 16; }

// ---- the chase.  A round stands on node pos -- which HAS a predecessor or is the start -- holds its {x, y}, writes the two words below to path[k .. k + 3]
// and goes on from p4 with k + 4 while p4 is a node.  Of what it wrote, the entries that count are pos and those of p1, p2, p3 that have a predecessor
// themselves (lattice.rs:150-152: BOS is not on the path, and neither is whatever else a chain ends in): as many as there are nodes among p1 .. p4.
KGPU_HD constexpr uint32_t bt_quad_word0(uint32_t pos, uint32_t y) { return pos | (y << 16); }          // path[k] = pos, path[k + 1] = p1
KGPU_HD constexpr uint32_t bt_quad_word1(uint32_t x, uint32_t y) { return (y >> 16) | (x << 16); }      // path[k + 2] = p2, path[k + 3] = p3
KGPU_HD constexpr uint32_t bt_quad_next(uint32_t x) { return x >> 16; }                                 // p4
KGPU_HD constexpr uint32_t bt_quad_count(uint32_t x, uint32_t y) {
    return (uint32_t)(bt_p1(y) != BT_NONE) + (uint32_t)(bt_p2(y) != BT_NONE) + (uint32_t)((x & 0xFFFFu) != BT_NONE) + (uint32_t)((x >> 16) != BT_NONE);
}
// The chase's loop runs while k <= C (a path has at most C + 1 entries: C words and EOS; the bound is never met on a well-formed lattice) and leaves with
// k_before = the entries in front of its LAST round and that round's {x, y}.  -> K.
KGPU_HD constexpr uint32_t bt_path_count(uint32_t k_before, uint32_t x, uint32_t y, uint32_t C) {
    const uint32_t k = k_before + bt_quad_count(x, y);
    return k < C + 1u ? k : C + 1u;
}
// What a round may write behind the path's last entry: path[] has C + 2 half-words and the last round starts at k <= C, k a multiple of BT_QUAD, so it ends
// in front of entry 4 floor(C / 4) + 4 <= C + 4 -- at most two half-words behind path[C + 1].
KGPU_HD constexpr uint32_t bt_path_overrun_bytes(uint32_t C) {
    const uint32_t end = BT_QUAD * (C / BT_QUAD) + BT_QUAD;
    return end > C + 2u ? 2u * (end - (C + 2u)) : 0u;
}
static_assert(bt_path_overrun_bytes(0) == 4 && bt_path_overrun_bytes(1) == 2 && bt_path_overrun_bytes(2) == 0 && bt_path_overrun_bytes(3) == 0 && bt_path_overrun_bytes(4) == 4, "overrun");
static_assert(bt_quad_count(0xFFFFFFFFu, 0xFFFFFFFFu) == 0 && bt_quad_count(0xFFFFFFFFu, 0xFFFF0007u) == 1 && bt_quad_count(0xFFFF0001u, 0x00030007u) == 3, "quad count");
static_assert(bt_hop(BT_NONE, 2) == 2 && bt_hop(1, 2) == 1 && bt_hop(BT_NONE, 0xFFFFu) == 0xFFFFu && bt_hop(0xFFFEu, 0xFFFFu) == 0xFFFEu, "hop");

}  // namespace kgpu
