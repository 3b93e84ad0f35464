// tests/c_abi/chunk_policy.cpp -- kanpyo_amd/csrc/kgpu_chunk_policy.h on the CPU (tests/test_chunk_policy_cpu.py builds this file with g++ alone: that the
// header needs nothing from HIP is part of the test).  The expected values were written out by hand from the loops the host calls carried before the two
// functions existed, and compared with those loops before they were deleted.
#include <cstdio>

#include "../../kanpyo_amd/csrc/kgpu_chunk_policy.h"

using namespace kgpu;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static bool step_is(ArenaDecision d, ArenaStep step, size_t want) { return d.step == step && d.want == want; }

int main() {
    // ---- the chunk cutter: (offsets, done, n, max sentences, max bytes) -> m
    const uint64_t tens[] = {0, 10, 20, 30, 40, 50};   // five sentences of 10 bytes
    CHECK(cut_chunk(tens, 0, 0, 4, 100) == 0);          // n = 0: no chunk
    CHECK(cut_chunk(tens, 5, 5, 4, 100) == 0);          // ... and nothing behind the last sentence
    const uint64_t big[] = {0, 100, 110, 120};
    CHECK(cut_chunk(big, 0, 3, 10, 50) == 1);           // a first sentence longer than the byte limit: a chunk of its own
    CHECK(cut_chunk(big, 1, 3, 10, 50) == 2);           // ... and the bytes count from the chunk's first sentence, not from the call's
    CHECK(cut_chunk(tens, 0, 4, 4, 1000) == 4);         // the sentence limit met exactly (n = limit)
    CHECK(cut_chunk(tens, 0, 5, 4, 1000) == 4);         // ... with a sentence left over
    CHECK(cut_chunk(tens, 4, 5, 4, 1000) == 1);         // ... which is the next chunk
    CHECK(cut_chunk(tens, 0, 5, 1, 1000) == 1);
    CHECK(cut_chunk(tens, 0, 5, 100, 20) == 2);         // the byte limit met exactly: 20 bytes fit 20
    CHECK(cut_chunk(tens, 0, 5, 100, 19) == 1);         // ... exceeded by one: the second sentence waits
    CHECK(cut_chunk(tens, 0, 5, 100, 21) == 2);
    CHECK(cut_chunk(tens, 1, 5, 100, 20) == 2);         // (done > 0: offsets[3] - offsets[1] = 20)
    CHECK(cut_chunk(tens, 1, 5, 100, 40) == 4);         // the call's end before either limit
    const uint64_t empties[] = {7, 7, 7, 7};
    CHECK(cut_chunk(empties, 0, 3, 100, 0) == 3);       // empty sentences cost no bytes
    CHECK(cut_chunk(tens, 0, 5, 0, 1000) == 0);         // (a sentence limit of 0 is the caller's to avoid: the hooks read 0 as "the default")

    // ---- the arena step: (limit, bytes allocated, largest arena, m) -> what next, and the size asked for
    CHECK(arena_share(0, 256) == 256 && arena_share(64, 256) == 64 && arena_share(512, 256) == 256 && arena_share(256, 256) == 256);
    CHECK(step_is(arena_step(0, 256, 1024, 4), ArenaStep::GROW, 512));       // limit 0: the whole arena doubles
    CHECK(step_is(arena_step(64, 256, 1024, 4), ArenaStep::GROW, 128));      // a set limit: the limit doubles, inside the arena that is there
    CHECK(step_is(arena_step(512, 256, 1024, 4), ArenaStep::GROW, 512));     // ... a limit above the arena: the arena's bytes count
    CHECK(step_is(arena_step(0, 512, 1024, 4), ArenaStep::GROW, 1024));      // want == the maximum: still grows
    CHECK(step_is(arena_step(0, 1024, 1024, 4), ArenaStep::HALVE, 2048));    // one doubling past it: the chunk in halves
    CHECK(step_is(arena_step(0, 1024, 1024, 2), ArenaStep::HALVE, 2048));
    CHECK(step_is(arena_step(0, 1024, 1024, 1), ArenaStep::GIVE_UP, 2048));  // m = 1 at the maximum: the sentence keeps its status
    CHECK(step_is(arena_step(512, 2048, 1024, 4), ArenaStep::GROW, 1024));   // the limit, not the (larger) arena, is what is compared with the maximum
    CHECK(step_is(arena_step(1024, 2048, 1024, 4), ArenaStep::HALVE, 2048));
    CHECK(step_is(arena_step(1024, 2048, 1024, 1), ArenaStep::GIVE_UP, 2048));
    CHECK(step_is(arena_step(0, 2048, 1024, 1), ArenaStep::GIVE_UP, 4096));  // (an arena already above a hooked maximum never grows)

    if (fails) { std::printf("FAILED %d\n", fails); return 1; }
    std::printf("ok chunk_policy\n");
    return 0;
}
