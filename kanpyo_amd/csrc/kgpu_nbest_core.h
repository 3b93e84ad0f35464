// kanpyo_amd/csrc/kgpu_nbest_core.h -- the rule of the N-best paths (include/kanpyo_gpu.h, "N-best paths"), written once for the host
// (kgpu_nbest_host.cpp: kgpu_nbest_host) and for the device (kgpu_nbest.hip): the same statements decide both.  Plain C++ without a HIP include.
//   the key        one entry (cost, pred, pred_rank) of a node's list as ONE 64-bit word whose unsigned order is the rule's lexicographic order:
//                  cost ^ 0x80000000 in the high word (int32 order as unsigned order), pred << 6 | pred_rank in the low word; all-ones = no entry
//   the candidate  a predecessor's entry + the target's word cost + the connection cost, int32; dropped at 1 << 30 and beyond
//   the record     the 24-byte kgpu_token of a node on a path, what tokenize emits for it
#pragma once
#include <cstdint>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_normalize_core.h"   // KGPU_NORM_HD

namespace kgpu {

constexpr uint64_t NBEST_NONE = ~0ull;              // no entry at this rank
constexpr int32_t NBEST_INF = 1 << 30;              // lattice.rs:117: what the reference's clamp and strict '<' keep out
constexpr uint32_t NBEST_RANK_BITS = 6;             // KGPU_NBEST_MAX = 64 ranks
constexpr uint64_t NBEST_MAX_NODES = 1ull << 26;    // pred << 6 | rank is 32 bits
static_assert(KGPU_NBEST_MAX == 1u << NBEST_RANK_BITS, "a rank is six bits of the key");

KGPU_NORM_HD uint64_t nbest_key(int32_t cost, uint32_t pred, uint32_t rank) {
    return ((uint64_t)((uint32_t)cost ^ 0x80000000u) << 32) | ((pred << NBEST_RANK_BITS) | rank);
}
KGPU_NORM_HD int32_t nbest_key_cost(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
KGPU_NORM_HD uint32_t nbest_key_pred(uint64_t key) { return (uint32_t)key >> NBEST_RANK_BITS; }
KGPU_NORM_HD uint32_t nbest_key_rank(uint64_t key) { return (uint32_t)key & (KGPU_NBEST_MAX - 1u); }
// L(BOS) = [(0, none, none)]: a key that is an entry (not all-ones) and is never followed -- a chain ends at node 0
KGPU_NORM_HD uint64_t nbest_bos_key() { return ((uint64_t)0x80000000u << 32) | 0xFFFFFFFFu; }

// The candidate (entry `pred_key` of predecessor `pred` at rank `rank`) -> target: its key, or NBEST_NONE where the predecessor has no such entry or the
// cost reaches 1 << 30.  An entry's cost is below 1 << 30 and the two addends are int16s: the int32 sum cannot wrap.
KGPU_NORM_HD uint64_t nbest_candidate(uint64_t pred_key, uint32_t pred, uint32_t rank, int32_t word_cost, int32_t conn_cost) {
    if (pred_key == NBEST_NONE) return NBEST_NONE;
    const int32_t cost = nbest_key_cost(pred_key) + word_cost + conn_cost;
    return cost >= NBEST_INF ? NBEST_NONE : nbest_key(cost, pred, rank);
}

// The record of a node: Token::new over the node's fields, and the EOS dummy as tokenizer.rs:27-28,34 makes it ("EOS" has three characters, no bytes).
KGPU_NORM_HD kgpu_token nbest_record(uint32_t cls, int32_t id, uint32_t byte_pos, uint32_t char_pos, uint32_t end_char, uint32_t byte_len) {
    if (cls == KGPU_CLASS_DUMMY) return kgpu_token{0, KGPU_CLASS_DUMMY, byte_pos, char_pos, char_pos + 3u, 0u};
    return kgpu_token{id, cls, byte_pos, char_pos, end_char, byte_len};
}

}  // namespace kgpu
