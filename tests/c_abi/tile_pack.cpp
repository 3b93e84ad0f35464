// tests/c_abi/tile_pack.cpp -- the stage-B address pack (kanpyo_amd/csrc/kgpu_tilepack.h) on the host: every 8-byte aligned node address against the
// extreme bucket addresses and the other way round, for both forms, up to each form's limit; what a form cannot hold it must say so (fits).
#include <cstdint>
#include <cstdio>

#include "../../kanpyo_amd/csrc/kgpu_tilepack.h"

using namespace kgpu;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 10) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

template <uint32_t SHIFT>
static uint64_t round_trips(uint32_t lds_bytes) {
    typedef TilePack<SHIFT> P;
    CHECK(P::fits(lds_bytes));
    const uint32_t top = lds_bytes - 8;   // the last aligned address of the allocation
    const uint32_t ext[] = {0u, 8u, 16u, 56u, 32760u, 32768u, 65528u < top ? 65528u : top, 65536u < top ? 65536u : top, 131064u < top ? 131064u : top,
                            131072u < top ? 131072u : top, top - 8, top};
    uint64_t n = 0;
    for (uint32_t x = 0; x <= top; x += 8)
        for (uint32_t e : ext) {
            const uint32_t w1 = P::pack(x, e), w2 = P::pack(e, x);
            CHECK(P::node_addr(w1) == x && P::bucket_addr(w1) == e);
            CHECK(P::node_addr(w2) == e && P::bucket_addr(w2) == x);
            n += 2;
        }
    return n;
}

int main() {
    // the limits themselves
    static_assert(TilePack<0>::limit == 64u * 1024u && TilePack<3>::limit == 512u * 1024u, "limits");
    static_assert(TilePack<0>::fits(64u * 1024u) && !TilePack<0>::fits(64u * 1024u + 8u), "the byte form ends at 64 KB");
    static_assert(!TilePack<0>::fits(80u * 1024u) && !TilePack<0>::fits(LDS_MAX_BYTES), "the byte form must refuse the large pools");
    static_assert(TilePack<3>::fits(LDS_MAX_BYTES) && !TilePack<3>::fits(512u * 1024u + 8u), "the unit form holds the chip's LDS and says where it ends");
    static_assert(TilePackLds::fits(LDS_MAX_BYTES), "the kernels' form holds every LDS size of the chip");
    static_assert(LDS_MAX_BYTES == 160u * 1024u, "gfx950");
    uint64_t n = 0;
    n += round_trips<0>(64u * 1024u);
    n += round_trips<0>(40u * 1024u);
    n += round_trips<3>(LDS_MAX_BYTES);
    n += round_trips<3>(80u * 1024u);
    n += round_trips<3>(64u * 1024u);
    n += round_trips<1>(128u * 1024u);
    n += round_trips<2>(LDS_MAX_BYTES);
    // what the byte form loses beyond its limit is why it has to refuse: the first address it cannot name aliases address 0
    CHECK(TilePack<0>::bucket_addr(TilePack<0>::pack(0u, 65536u)) != 65536u);
    CHECK(TilePack<0>::node_addr(TilePack<0>::pack(65536u, 0u)) != 65536u || TilePack<0>::bucket_addr(TilePack<0>::pack(65536u, 0u)) != 0u);
    // the kernels' form: the product's and the tests' pool sizes, every address, both ends of the other half-word (done above); spot values
    CHECK(TilePackLds::pack(8u, 0u) == 1u && TilePackLds::pack(0u, 8u) == 0x10000u);
    CHECK(TilePackLds::pack(LDS_MAX_BYTES - 8, LDS_MAX_BYTES - 8) == 0x4FFF4FFFu);
    if (fails) { printf("FAIL %d checks\n", fails); return 1; }
    printf("ok %llu round trips\n", (unsigned long long)n);
    return 0;
}
