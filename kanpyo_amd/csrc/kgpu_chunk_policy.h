// kanpyo_amd/csrc/kgpu_chunk_policy.h -- two decisions of the chunked host calls as pure functions: where a chunk ends, and what a chunk whose kept lattices
// overflowed the arena does next.  Includes nothing from HIP (tests/c_abi/chunk_policy.cpp builds it with g++ alone, as kgpu_chain.h is built).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace kgpu {

// The sentences of the chunk that begins at sentence `done` of n: at most max_sents, and at most max_bytes of input -- but never none while sentences are
// left: a first sentence longer than max_bytes is a chunk of its own.  offsets: n + 1 entries.
inline uint64_t cut_chunk(const uint64_t *offsets, uint64_t done, uint64_t n, uint64_t max_sents, uint64_t max_bytes) {
    uint64_t m = 0;
    while (done + m < n && m < max_sents && (m == 0 || offsets[done + m + 1] - offsets[done] <= max_bytes)) ++m;
    return m;
}

// What of the arena a chunk's kept lattices may use: `limit` (a test hook; 0: none) caps it below the bytes allocated.
inline size_t arena_share(size_t limit, size_t arena_bytes) { return limit ? std::min(limit, arena_bytes) : arena_bytes; }

// A chunk of m sentences did not fit its share of the arena (the arena_overflow protocol): twice the share while that stays within arena_max (GROW: the
// arena is made `want` bytes, a set limit becomes `want`, the chunk runs once more); at the largest arena the chunk in halves (HALVE); and a single sentence
// that does not fit there keeps KGPU_SENT_NO_SCRATCH (GIVE_UP).
enum class ArenaStep { GROW, HALVE, GIVE_UP };
struct ArenaDecision { ArenaStep step; size_t want; };
inline ArenaDecision arena_step(size_t limit, size_t arena_bytes, size_t arena_max, uint64_t m) {
    const size_t want = arena_share(limit, arena_bytes) * 2;
    if (want <= arena_max) return {ArenaStep::GROW, want};
    return {m > 1 ? ArenaStep::HALVE : ArenaStep::GIVE_UP, want};
}

}  // namespace kgpu
