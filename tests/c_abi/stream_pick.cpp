// pick_stream (kanpyo_amd/csrc/kgpu_chain.cpp) on the CPU, no device: which of a dictionary's shared streams a batch goes to, by the load the host
// knows of.  tests/test_stream_pick_cpu.py builds this file with g++ against kgpu_chain.cpp alone.  Prints "ok <checks>" or FAIL lines.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_chain.h"

using namespace kgpu;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) { ++failures; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// A dictionary's shared streams as kgpu_ctx.cpp keeps them: a batch adds its weight to the stream it is given, its retirement takes it off again.
struct Streams {
    std::atomic<uint64_t> load[8];
    std::atomic<unsigned> cursor{0};
    unsigned n;
    explicit Streams(unsigned n_) : n(n_) { for (auto &l : load) l.store(0); }
    unsigned give(uint64_t weight) { const unsigned s = pick_stream(load, n, cursor); load[s].fetch_add(weight); return s; }
    void retire(unsigned s, uint64_t weight) { load[s].fetch_sub(weight); }
};

int main() {
    const uint64_t FULL = stream_batch_weight(4096 * 113), TAIL = stream_batch_weight(1696 * 113);
    CHECK(stream_batch_weight(0) > 0);                       // an empty batch counts
    CHECK(TAIL < FULL && TAIL * 2 < FULL + TAIL);            // a tail batch weighs what it costs
    for (unsigned n : {3u, 4u}) {   // equal weights, nothing retired: strict rotation from the cursor
        Streams s(n);
        for (unsigned b = 0; b < 5 * n; ++b) CHECK(s.give(FULL) == b % n);
        for (unsigned k = 0; k < n; ++k) CHECK(s.load[k].load() == 5 * FULL);
    }
    for (unsigned n : {3u, 4u}) {   // ... and with every batch retired before the next is picked (one context): rotation all the same
        Streams s(n);
        for (unsigned b = 0; b < 5 * n; ++b) { const unsigned got = s.give(FULL); CHECK(got == b % n); s.retire(got, FULL); }
    }
    {   // eight contexts as bench_engine.GpuEngine drives them, three streams, equal batches: context b mod 8 retires batch b - 8 just before batch b is picked
        Streams s(3);
        std::vector<unsigned> where;
        for (unsigned b = 0; b < 8 * 24; ++b) {
            if (b >= 8) s.retire(where[b - 8], FULL);
            where.push_back(s.give(FULL));
            if (b >= 8) {   // seven batches are known in flight beside the new one: no stream holds more than three
                for (unsigned k = 0; k < 3; ++k) CHECK(s.load[k].load() <= 3 * FULL);
                CHECK(s.load[0].load() + s.load[1].load() + s.load[2].load() == 8 * FULL);
            }
            if (b >= 23) {  // any 24 consecutive picks: 8 / 8 / 8
                unsigned got[3] = {0, 0, 0};
                for (unsigned k = b - 23; k <= b; ++k) ++got[where[k]];
                CHECK(got[0] == 8 && got[1] == 8 && got[2] == 8);
            }
        }
    }
    {   // the same with a whole step retired at once (the engine's results()): 8 / 8 / 8 again
        Streams s(3);
        unsigned got[3] = {0, 0, 0};
        for (unsigned step = 0; step < 3; ++step) {
            unsigned where[8];
            for (unsigned b = 0; b < 8; ++b) { where[b] = s.give(FULL); ++got[where[b]]; }
            for (unsigned b = 0; b < 8; ++b) s.retire(where[b], FULL);
        }
        CHECK(got[0] == 8 && got[1] == 8 && got[2] == 8);
    }
    {   // a batch of 1696 sentences among batches of 4096: the bytes decide, not the count
        Streams s(3);
        CHECK(s.give(FULL) == 0);
        CHECK(s.give(TAIL) == 1);
        CHECK(s.give(FULL) == 2);
        CHECK(s.give(FULL) == 1);          // one full and one tail batch there: still the least
        CHECK(s.give(FULL) == 2);          // the cursor is at 2, streams 0 and 2 tie at one full batch
        CHECK(s.give(FULL) == 0);          // full | tail + full | 2 full: stream 0
        CHECK(s.give(TAIL) == 1);          // 2 full | tail + full | 2 full: stream 1
        CHECK(s.load[1].load() == 2 * TAIL + FULL && s.load[0].load() == 2 * FULL && s.load[2].load() == 2 * FULL);
        // by count stream 1 holds three, the others two; by bytes it is lighter by less than an eighth (2 x 1696 against 4096): a tie, the cursor's stream
        CHECK(2 * TAIL < FULL && (2 * TAIL + FULL) + (2 * TAIL + FULL) / STREAM_TIE_SHARE >= 2 * FULL);
        CHECK(s.cursor.load() == 2 && s.give(FULL) == 2);
        // ... and with the next full batch on each of the others it is lighter by more than that
        CHECK(s.give(FULL) == 0);
        CHECK(s.give(FULL) == 1);
    }
    {   // the chunks of a large host call: ten in flight on three streams, retired in order, their bytes a few per cent apart -- a tie every time: rotation
        Streams s(3);
        std::vector<unsigned> where;
        std::vector<uint64_t> w;
        uint32_t x = 12345;
        for (unsigned b = 0; b < 200; ++b) {
            x = x * 1664525u + 1013904223u;
            w.push_back(stream_batch_weight(16384 * 113) * (970 + (x >> 16) % 61) / 1000);   // +- 3 %
            if (b >= 10) s.retire(where[b - 10], w[b - 10]);
            where.push_back(s.give(w[b]));
            CHECK(where[b] == b % 3);
        }
    }
    {   // a single stream
        Streams s(1);
        for (int b = 0; b < 4; ++b) CHECK(s.give(b ? FULL : 0) == 0);
        CHECK(s.cursor.load() == 0);
    }
    {   // the cursor wraps, and one beyond the streams is taken modulo their number
        Streams s(3);
        s.cursor.store(2);
        CHECK(s.give(FULL) == 2 && s.cursor.load() == 0);
        CHECK(s.give(FULL) == 0 && s.cursor.load() == 1);
        Streams t(3);
        t.cursor.store(0xFFFFFFFFu);       // 2^32 - 1 = 0 (mod 3)
        CHECK(t.give(FULL) == 0 && t.cursor.load() == 1);
        Streams u(4);
        u.cursor.store(7);
        CHECK(u.give(FULL) == 3 && u.cursor.load() == 0);
    }
    {   // the least-loaded stream wins wherever the cursor stands; ties go to the first at or after the cursor
        Streams s(4);
        s.load[0] = 5; s.load[1] = 3; s.load[2] = 9; s.load[3] = 3;
        s.cursor.store(2);
        CHECK(s.give(0) == 3 && s.cursor.load() == 0);
        CHECK(s.give(0) == 1 && s.cursor.load() == 2);
        s.cursor.store(1);
        CHECK(s.give(1) == 1);             // 5 4 9 3 next
        CHECK(s.give(0) == 3);
    }
    {   // a load that returns to zero: the stream is taken again, and nothing wraps below zero
        Streams s(3);
        const unsigned a = s.give(FULL), b = s.give(TAIL), c = s.give(0);
        CHECK(a == 0 && b == 1 && c == 2);
        s.retire(a, FULL); s.retire(b, TAIL); s.retire(c, 0);
        for (unsigned k = 0; k < 3; ++k) CHECK(s.load[k].load() == 0);
        CHECK(s.give(FULL) == 0);          // the cursor had wrapped to 0
        s.retire(0, FULL);
        CHECK(s.load[0].load() == 0 && s.give(FULL) == 1);
    }
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
