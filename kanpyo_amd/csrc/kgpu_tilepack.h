// kanpyo_amd/csrc/kgpu_tilepack.h -- the two LDS addresses of a stage-B tile in ONE 32-bit word (kgpu_device.h: the gather computes a tile's node and
// bucket address once and hands both to the sweep in a single register).  No HIP in here: the same code is compiled for the host by
// tests/test_tile_pack_cpu.py.
//
// Both addresses are 8-byte aligned (node[] and bk[] hold uint2 entries at 8-byte aligned bases, the lane offsets are multiples of 8), so a half-word
// holds an address in units of 2^SHIFT bytes, SHIFT <= 3:
//   SHIFT = 0: byte addresses -- pack is one shift-or, unpack an `and` and a shift; holds LDS addresses below 64 KB only;
//   SHIFT = 3: 8-byte units -- one shift more in the pack; holds addresses below 512 KB, i.e. every LDS size of the chip (160 KB per workgroup).
// Both LDS kernels use SHIFT = 3 (TilePackLds): the pool kernel runs with pools of up to 160 KB (KGPU_POOL=160:4) and one instantiation serves every
// shape -- a byte-form twin of the kernel for launches of at most 64 KB would save one VALU instruction per tile and cost a second copy of every
// instantiation.  `fits` is what a launch has to check for a form: the static_assert below holds SHIFT = 3 against the chip's LDS, and the
// launches check the LDS size they request (launch_tokenize_pool, launch_tokenize_window).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KGPU_HD __host__ __device__ __forceinline__
#else
#define KGPU_HD inline
#endif

namespace kgpu {

template <uint32_t SHIFT>
struct TilePack {
    static_assert(SHIFT <= 3, "node and bucket entries are 8-byte aligned, not more");
    static constexpr uint32_t unit = 1u << SHIFT;
    static constexpr uint32_t limit = 65536u << SHIFT;   // the first LDS address a half-word cannot name
    // every address inside an LDS allocation of `lds_bytes` (addresses 0 .. lds_bytes - 1) can be packed
    static constexpr bool fits(uint32_t lds_bytes) { return lds_bytes <= limit; }
    // na, ba: multiples of 8 below `limit`
    static KGPU_HD constexpr uint32_t pack(uint32_t na, uint32_t ba) { return (na >> SHIFT) | (ba << (16u - SHIFT)); }
    static KGPU_HD constexpr uint32_t node_addr(uint32_t w) { return (w & 0xFFFFu) << SHIFT; }
    static KGPU_HD constexpr uint32_t bucket_addr(uint32_t w) { return (w >> 16) << SHIFT; }
};

// ---- how many tiles a start position has.  A tile is up to TILE_DIM targets x TILE_DIM predecessors; a position with T targets (nodes that start there)
// and P predecessors (nodes that end there) is ceil(T / 8) target groups x ceil(P / 8) predecessor chunks.  P = 0 -- nothing ends at the position -- is NO
// tile: every target's result is known without a sweep (dp = INF, no best predecessor: lattice.rs:116-142 with an empty edges[pos]) and the kernel's emit
// phase writes it.  The kernel's scan (how many descriptors a sentence has, where a position's start) and its list builder (tile_groups(P) chunks for each
// of the target groups) both go through these two, so the list is exactly as long as the scan said: tests/test_tile_count_cpu.py.
constexpr uint32_t TILE_DIM = 8;
KGPU_HD constexpr uint32_t tile_groups(uint32_t n) { return (n + TILE_DIM - 1u) / TILE_DIM; }   // chunks of n predecessors, groups of n targets; 0 -> 0
KGPU_HD constexpr uint32_t tile_count(uint32_t T, uint32_t P) { return tile_groups(T) * tile_groups(P); }   // = P ? ceil(T / 8) * ceil(P / 8) : 0
static_assert(tile_count(1, 0) == 0 && tile_count(0, 5) == 0 && tile_count(1, 1) == 1 && tile_count(9, 8) == 2 && tile_count(17, 9) == 6, "tile_count");

constexpr uint32_t LDS_MAX_BYTES = 160u * 1024u;   // per workgroup on gfx950
typedef TilePack<3> TilePackLds;
static_assert(TilePackLds::fits(LDS_MAX_BYTES), "the unit form must hold every LDS address of the chip");
static_assert(!TilePack<0>::fits(LDS_MAX_BYTES) && TilePack<0>::fits(64u * 1024u), "the byte form ends at 64 KB");

}  // namespace kgpu
