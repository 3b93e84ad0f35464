// kanpyo_amd/csrc/kgpu_user_core.h -- the rule of the user dictionary (include/kanpyo_gpu.h, "user dictionary"), written once for the host
// (kgpu_user_host.cpp: kgpu_userdict_host) and for the device (kgpu_user.hip): the same statements decide both.  Plain C++ without a HIP include.
//   the table      the entries' distinct keys in an open-addressed table of 64-bit tags (hash << 32 | group + 1), a group per distinct key with its
//                  entries side by side in ascending entry order: user_find confirms every hit by comparing bytes, so no answer depends on a slot's place
//   the match      user_match: the groups whose key stands at a character position, by the key lengths that exist (a 64-bit mask), shortest first
//   the withdrawal user_withdrawn: which positions lose their Unknown nodes, and USER_WITHDRAWN, the state word of such a node
//   the record     user_record; everything else (penalty, candidate, key, state, record count) is kgpu_mode_core.h's, over the widened node set
#pragma once
#include <cstdint>

#include "kgpu_mode_core.h"

namespace kgpu {

constexpr uint32_t USER_MAX_KEY_CHARS = 64, USER_MAX_KEY_BYTES = 255;
constexpr uint32_t USER_NO_GROUP = 0xFFFFFFFFu;
constexpr uint64_t USER_MAX_NODES = MODE_MAX_NODES;   // lattice and user nodes together: a combined index is the low word of a key
// The state word of a withdrawn node: dp -1 with no predecessor, which mode_state never makes (it gives 1 << 30 with None, and BOS is 0 with None).
constexpr uint64_t USER_WITHDRAWN = ~0ull;

struct alignas(16) UserGroup { uint32_t key_off, key_bytes, first, count; };   // the key's bytes in the arena; its entries are ents[first .. first + count)
struct alignas(16) UserEntry { uint32_t entry, ids; int32_t cost; uint32_t pad; };   // e; left id | right id << 16 as the connection matrix in use numbers them
struct UserTableView {
    const uint64_t *slots; uint32_t slot_mask;   // a power of two of slots; 0: an empty one
    const UserGroup *groups;
    const UserEntry *ents;
    const uint8_t *arena;                        // the distinct keys back to back
    uint64_t len_mask;                           // bit L - 1: some key has L characters
    uint32_t n_entries, n_groups;
};

// FNV-1a over the bytes, then murmur3's finaliser with the length folded in: the value of key_hash (kgpu_records_dev.h) and vocab_key_hash
// (kgpu_vocab_table.cpp), the hash of the other byte-keyed tables.
KGPU_NORM_HD uint32_t user_key_hash(const uint8_t *p, uint32_t len) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < len; ++i) h = (h ^ p[i]) * 16777619u;
    h ^= len;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
KGPU_NORM_HD uint64_t user_slot_tag(uint32_t hash, uint32_t group) { return ((uint64_t)hash << 32) | (group + 1u); }

// The group whose key is the len bytes at p, or USER_NO_GROUP.  Linear probing from the hash's slot up to the first empty slot (the table is at most half
// full); a tag's hash selects, the bytes decide.
KGPU_NORM_HD uint32_t user_find(const UserTableView &t, const uint8_t *p, uint32_t len) {
    if (!t.n_groups || len > USER_MAX_KEY_BYTES) return USER_NO_GROUP;
    const uint32_t h = user_key_hash(p, len);
    for (uint32_t at = h & t.slot_mask, probes = 0; probes <= t.slot_mask; at = (at + 1) & t.slot_mask, ++probes) {
        const uint64_t tag = t.slots[at];
        if (!tag) return USER_NO_GROUP;
        if ((uint32_t)(tag >> 32) != h) continue;
        const uint32_t g = (uint32_t)tag - 1u;
        const UserGroup gr = t.groups[g];
        if (gr.key_bytes != len) continue;
        const uint8_t *k = t.arena + gr.key_off;
        uint32_t i = 0;
        while (i < len && k[i] == p[i]) ++i;
        if (i == len) return g;
    }
    return USER_NO_GROUP;
}

// The groups whose key stands at character position q of a sentence of C characters (cbyte: every position's byte offset, [C] = the bytes): visit(group,
// characters) per hit, shortest key first -> the entries that match there.  Work: one probe per key length that exists and still fits.
template <class F>
KGPU_NORM_HD uint32_t user_match(const UserTableView &t, const uint8_t *text, const uint32_t *cbyte, uint32_t C, uint32_t q, F &&visit) {
    uint32_t hits = 0;
    const uint32_t b0 = cbyte[q];
    for (uint64_t m = t.len_mask; m; m &= m - 1) {
        const uint32_t L = (uint32_t)__builtin_ctzll(m) + 1u;
        if (L > C - q) break;
        const uint32_t g = user_find(t, text + b0, cbyte[q + L] - b0);
        if (g == USER_NO_GROUP) continue;
        hits += t.groups[g].count;
        visit(g, L);
    }
    return hits;
}

// The entries of a group (n of them at ents, in ascending entry order) whose entry index is below e: where an entry of ANOTHER group of the same start
// position goes among them -- a node's rank among its position's nodes is the sum of these over the position's groups (entry indices are distinct).
KGPU_NORM_HD uint32_t user_entries_below(const UserEntry *ents, uint32_t n, uint32_t e) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ents[mid].entry < e) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The Unknown lattice nodes that start at a position are withdrawn iff an entry matches there, no Known lattice node starts there and the category of the
// character there does not invoke unknown words on its own (reference src/lattice.rs:54: an entry behaves as a word of the dictionary would).
KGPU_NORM_HD bool user_withdrawn(uint32_t matches, bool known_starts, bool invoke) { return matches != 0 && !known_starts && !invoke; }

// The record of the user node of entry e over characters [start, end).
KGPU_NORM_HD kgpu_token user_record(uint32_t e, uint32_t byte_pos, uint32_t start, uint32_t end, uint32_t byte_len) {
    return kgpu_token{(int32_t)(e + 1u), KGPU_CLASS_USER, byte_pos, start, end, byte_len};
}

}  // namespace kgpu
