// tests/c_abi/pack_sanitize.cpp -- kgpu_pack_host (kanpyo_amd/csrc/kgpu_pack_rule.cpp, compiled beside this file without HIP) on the extreme shapes of
// the CPU sweep, with every buffer allocated at its exact size: built with -fsanitize=address,undefined and run as it is, a read or a store one element
// outside any array ends the program.  Prints "pack sanitized ok <calls> <rows>".  Checks besides: the capacity protocol (one row short: nothing is
// written), the total equals the last offset, every row's mask is a prefix of ones, and bad offsets are refused without a read.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kanpyo_gpu.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (the library's writes a thread-local message)
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "pack_sanitize: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

int main() {
    const uint32_t lengths[] = {3, 4, 5, 7, 8, 16, 17, 64, 65, 512};
    uint64_t calls = 0, rows_total = 0;
    for (uint32_t ML : lengths)
        for (int pair = 0; pair < 2; ++pair)
            for (uint32_t strategy = 0; strategy < 3; ++strategy)
                for (uint32_t windows = 0; windows < 2; ++windows)
                    for (uint32_t trims = 0; trims < 4; ++trims) {
                        const uint32_t ns = pair ? 3 : 2;
                        if (ML < ns + 1 || (strategy == KGPU_PACK_ONLY_SECOND && !pair) || (strategy == KGPU_PACK_LONGEST_FIRST && windows)) continue;
                        const uint32_t room = ML - ns, tf = trims & 1, tb = trims >> 1;
                        const uint32_t strides[] = {0, 1, room - 1, room > 2 ? room - 2 : 0};
                        for (uint32_t stride : strides) {
                            if (stride >= room) continue;
                            const uint64_t step = room - stride;
                            const uint64_t lens[] = {0, 1, room - 1, room, room + 1ull, room + step, 3ull * room};
                            // the samples: every pair of lengths (singles: every length), plus sequences shorter than their trims
                            std::vector<int32_t> ids;
                            std::vector<uint64_t> off_a(1, 0), off_b;
                            std::vector<uint64_t> la, lb;
                            for (uint64_t a : lens)
                                for (uint64_t b : lens) { la.push_back(a + tf + tb); lb.push_back(b + tf + tb); if (!pair) break; }
                            la.push_back(0); lb.push_back(1); la.push_back(1); lb.push_back(0);
                            const size_t n = la.size();
                            ids.push_back((int32_t)rnd());   // (the first sequence does not start at 0)
                            off_a[0] = 1;
                            for (size_t i = 0; i < n; ++i) { for (uint64_t k = 0; k < la[i]; ++k) ids.push_back((int32_t)rnd()); off_a.push_back(ids.size()); }
                            if (pair) {
                                off_b.push_back(ids.size());
                                for (size_t i = 0; i < n; ++i) { for (uint64_t k = 0; k < lb[i]; ++k) ids.push_back((int32_t)rnd()); off_b.push_back(ids.size()); }
                            }
                            const uint64_t n_in = ids.size();
                            std::vector<kgpu_span> spans_in(n_in);
                            std::vector<int32_t> tix_in(n_in);
                            for (uint64_t e = 0; e < n_in; ++e) { spans_in[e] = kgpu_span{rnd(), rnd(), rnd(), rnd()}; tix_in[e] = (int32_t)rnd(); }
                            kgpu_pack_opts o{(uint32_t)sizeof(kgpu_pack_opts), windows ? KGPU_PACK_WINDOWS : 0u, strategy, ML, stride, -7, -8, -9, tf, tb};
                            std::vector<uint64_t> roff(n + 1);
                            std::vector<uint8_t> status(n);
                            uint64_t need = 0;
                            // no capacity at all: the count, and no store
                            int rc = kgpu_pack_host(&o, n, ids.data(), off_a.data(), pair ? ids.data() : nullptr, pair ? off_b.data() : nullptr, n_in, spans_in.data(),
                                                    tix_in.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, roff.data(), status.data(), &need);
                            REQUIRE(rc == KGPU_ERR_CAPACITY && need > 0 && roff[n] == need);
                            // one row short: still nothing is written (the buffers hold need - 1 rows exactly)
                            {
                                const uint64_t cap = need - 1;
                                std::vector<int32_t> x(cap * ML, 0x5A5A5A5A);
                                uint64_t got = 0;
                                rc = kgpu_pack_host(&o, n, ids.data(), off_a.data(), pair ? ids.data() : nullptr, pair ? off_b.data() : nullptr, n_in, nullptr, nullptr,
                                                    x.data(), nullptr, nullptr, nullptr, nullptr, cap, roff.data(), status.data(), &got);
                                REQUIRE(rc == KGPU_ERR_CAPACITY && got == need);
                                for (int32_t v : x) REQUIRE(v == 0x5A5A5A5A);
                            }
                            // the exact capacity: everything is written, nothing beyond
                            std::vector<int32_t> in_ids(need * ML), types(need * ML), mask(need * ML), tix(need * ML);
                            kgpu_span *spans = (kgpu_span *)std::aligned_alloc(16, need * ML * sizeof(kgpu_span));   // (exactly the rows: the sanitizer guards its end)
                            uint64_t got = 0;
                            rc = kgpu_pack_host(&o, n, ids.data(), off_a.data(), pair ? ids.data() : nullptr, pair ? off_b.data() : nullptr, n_in, spans_in.data(),
                                                tix_in.data(), in_ids.data(), types.data(), mask.data(), spans, tix.data(), need, roff.data(), status.data(), &got);
                            REQUIRE(rc == KGPU_OK && got == need && roff[n] == need && roff[0] == 0);
                            for (uint64_t r = 0; r < need; ++r) {
                                REQUIRE(in_ids[r * ML] == -7 && mask[r * ML] == 1);
                                for (uint32_t j = 1; j < ML; ++j) {
                                    REQUIRE(mask[r * ML + j] <= mask[r * ML + j - 1]);   // ones, then zeros
                                    if (!mask[r * ML + j]) REQUIRE(in_ids[r * ML + j] == -9 && types[r * ML + j] == 0 && tix[r * ML + j] == -1);
                                }
                            }
                            std::free(spans);
                            // rule 8: a range past n_ids_in, and one that runs backwards, are refused -- with n_ids_in cut the arrays ARE that short
                            if (n_in > 1) {
                                std::vector<int32_t> few(ids.begin(), ids.begin() + (n_in - 1));
                                rc = kgpu_pack_host(&o, n, few.data(), off_a.data(), pair ? few.data() : nullptr, pair ? off_b.data() : nullptr, n_in - 1, nullptr, nullptr,
                                                    in_ids.data(), nullptr, nullptr, nullptr, nullptr, need, roff.data(), status.data(), &got);
                                REQUIRE(rc == KGPU_ERR_INVALID_ARG);
                                std::vector<uint64_t> back(off_a);
                                back[1] = 0;   // (sample 0 runs from 1 back to 0)
                                rc = kgpu_pack_host(&o, n, ids.data(), back.data(), pair ? ids.data() : nullptr, pair ? off_b.data() : nullptr, n_in, nullptr, nullptr,
                                                    in_ids.data(), nullptr, nullptr, nullptr, nullptr, need, roff.data(), status.data(), &got);
                                REQUIRE(rc == KGPU_ERR_INVALID_ARG);
                            }
                            ++calls;
                            rows_total += need;
                        }
                    }
    std::printf("pack sanitized ok %llu %llu\n", (unsigned long long)calls, (unsigned long long)rows_total);
    return 0;
}
