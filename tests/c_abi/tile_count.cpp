// tests/c_abi/tile_count.cpp -- the stage-B tile count (kanpyo_amd/csrc/kgpu_tilepack.h: tile_groups, tile_count) on the host, against counts made the
// long way for T, P in 0..40: the pairs covered by tiles of 8 x 8, and the descriptors the pool kernel's list builder writes (tile_groups(P) chunks for
// every group of 8 targets, none for a position nothing ends at) -- the scan's count and the builder's list must be the same length.
#include <cstdint>
#include <cstdio>

#include "../../kanpyo_amd/csrc/kgpu_tilepack.h"

using namespace kgpu;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 10) printf("FAIL %s:%d %s (T %u P %u)\n", __FILE__, __LINE__, #c, T, P); } } while (0)

// every (target, predecessor) pair marks the tile it falls into: distinct tiles touched
static uint32_t brute_tiles(uint32_t T, uint32_t P) {
    bool hit[8][8] = {};
    uint32_t n = 0;
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t p = 0; p < P; ++p)
            if (!hit[t / 8][p / 8]) { hit[t / 8][p / 8] = true; ++n; }
    return n;
}

// the list builder's loops (kgpu_pool.hip, emit 3c), counting instead of writing; also checks what a descriptor would hold
static uint32_t builder_tiles(uint32_t T_in, uint32_t P, uint64_t &pairs) {
    const uint32_t T = P ? T_in : 0u;
    const uint32_t kb = tile_groups(P);
    uint32_t k = 0;
    pairs = 0;
    for (uint32_t ta = 0; ta < T; ta += 8)
        for (uint32_t b = 0;;) {
            const uint32_t Tt = T - ta < 8u ? T - ta : 8u, Pt = P - 8 * b < 8u ? P - 8 * b : 8u;
            if (Tt < 1 || Tt > 8 || Pt < 1 || Pt > 8) return 0xFFFFFFFFu;   // a descriptor holds Tt - 1 and Pt - 1 in three bits each
            pairs += (uint64_t)Tt * Pt;
            ++k;
            if (++b >= kb) break;
        }
    return k;
}

int main() {
    static_assert(TILE_DIM == 8, "the kernels' tiles are 8 x 8: lane = 8 ti + j");
    static_assert(tile_count(0, 0) == 0 && tile_count(40, 0) == 0 && tile_count(0, 40) == 0, "no targets or no predecessors: no tile");
    static_assert(tile_count(8, 8) == 1 && tile_count(9, 8) == 2 && tile_count(8, 9) == 2 && tile_count(40, 40) == 25, "spot values");
    uint64_t n = 0;
    for (uint32_t T = 0; T <= 40; ++T)
        for (uint32_t P = 0; P <= 40; ++P) {
            const uint32_t want = P ? ((T + 7) / 8) * ((P + 7) / 8) : 0u;   // the definition
            CHECK(tile_count(T, P) == want);
            CHECK(tile_count(T, P) == brute_tiles(T, P));
            CHECK(tile_count(T, P) == tile_groups(T) * tile_groups(P));
            uint64_t pairs = 0;
            CHECK(builder_tiles(T, P, pairs) == tile_count(T, P));
            CHECK(pairs == (uint64_t)T * P);   // every relaxation of the position in exactly one tile
            CHECK((tile_count(T, P) == 0) == (T == 0 || P == 0));
            ++n;
        }
    if (fails) { printf("FAIL %d checks\n", fails); return 1; }
    printf("ok %llu shapes\n", (unsigned long long)n);
    return 0;
}
