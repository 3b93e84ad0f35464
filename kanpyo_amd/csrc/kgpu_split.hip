// kanpyo_amd/csrc/kgpu_split.hip -- the CLI's read_line + trim_end (reference src/bin/kanpyo.rs:114-122) over a block of bytes in HBM:
// lines end at '\n' only, each loses its trailing Unicode White_Space (complete encodings on bytes, include/kanpyo_gpu.h), the trimmed
// lines are packed back to back and delimited by u64 offsets.  Position-parallel, no backward walk over a line:
//   S[i]     byte i lies inside an occurrence of one of the White_Space encodings (1, 2 or 3 bytes; from bytes i - 2 .. i + 2)
//   kept[i]  the first non-S byte at or after i comes before the first '\n' at or after i (the end of the block counts as a '\n')
// An "event" is a byte that is '\n' or not S.  A byte is kept when the first event at or after it is a non-space; a run of spaces that
// reaches the end of a tile takes the answer of the first later tile that has an event -- one flag per tile.
//
// A tile is TILE = 4096 bytes of the ADDRESS space (16-byte aligned units, so the tile size is a multiple of 16): 256 lanes x one
// 16-byte load (16384-byte tiles on 1024 lanes: the carry kernel 36 -> 8.5 us at 64 MiB, but reduce 67 -> 88 and apply 80 -> 117 us).
// Three launches on the context's stream, none waits for another workgroup:
//   k_split_reduce  one workgroup per tile -> agg[t] = {newlines, bytes kept whatever follows the tile, length of the run of spaces
//                   at the tile's end, kind of the tile's first event (0 '\n', 1 non-space, 2 none)}
//   k_split_carry   one workgroup, in place over agg: backwards, the flag of every tile (the kind of the first event behind it);
//                   forwards, the exclusive sums of newlines and of kept bytes (kept = the tile's own + its trailing run if the flag
//                   says so): agg[t] = {newlines before, kept bytes before, -, flag}; agg[ntiles] = {newlines, kept bytes, lines};
//                   offsets[0], the last line's end when it has no '\n', and the two counts published to the host's mapped words
//   k_split_apply   one workgroup per tile: the tile again (L2 / Infinity-Cache resident for CLI-sized blocks), kept bytes compacted
//                   into LDS in order and stored as aligned 16-byte units (bytes at the run's two ends); offsets[rank + 1] of each
//                   '\n'.  Nothing is stored when the line count does not fit offsets_capacity.
// The input is read twice, the kept bytes and the offsets written once: about 3 bytes moved per input byte.
#include <hip/hip_runtime.h>

#include "kgpu_device.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TILE = 4096;          // bytes per workgroup: 256 lanes x 16 (a multiple of 16)
constexpr uint32_t THREADS = TILE / 16;
constexpr uint32_t WAVES = THREADS / 64;

// Four aligned bytes at address-space position q (a multiple of 4) of the block, zero where the block has none (a zero byte is neither
// space nor part of an encoding of one).  lo / hi: the block is [lo, hi) there.
__device__ __forceinline__ uint32_t load_word(const uint8_t *abase, uint64_t q, uint64_t lo, uint64_t hi) {
    if (q >= lo && q + 4 <= hi) return *(const uint32_t *)(abase + q);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (q + b >= lo && q + b < hi) v |= (uint32_t)abase[q + b] << (8 * b);
    return v;
}

// One lane's 16 bytes.  w: the bytes; ns / nl / vm: 16-bit masks over them -- not White_Space, '\n', inside the block (ns and nl are
// subsets of vm).
struct Unit { uint32_t w[4], ns, nl, vm; };

__device__ __forceinline__ bool space3(uint32_t t) {   // t = b0 | b1 << 8 | b2 << 16
    const uint32_t d = t - 0x8080E2u;                  // E2 80 80 .. E2 80 8A: U+2000-200A
    return ((d & 0xFFFFu) == 0 && d <= 0x0A0000u) || t == 0x809AE1u /* U+1680 */ || t == 0xA880E2u || t == 0xA980E2u /* U+2028, 2029 */ ||
           t == 0xAF80E2u /* U+202F */ || t == 0x9F81E2u /* U+205F */ || t == 0x8080E3u /* U+3000 */;
}

__device__ __forceinline__ Unit load_unit(const SplitArgs &a, uint64_t q) {   // q: address-space position of the unit, a multiple of 16
    const uint64_t mis = (uint64_t)(uintptr_t)a.in & 15u, lo = mis, hi = mis + a.len;
    const uint8_t *abase = a.in - mis;
    Unit u;
    uint32_t W[6];   // bytes q - 4 .. q + 20: the unit and a word on each side
    if (q >= lo && q + 16 <= hi) {
        const uint4 v = *(const uint4 *)(abase + q);
        W[1] = v.x; W[2] = v.y; W[3] = v.z; W[4] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) W[1 + k] = load_word(abase, q + 4 * k, lo, hi);
    }
    W[0] = q >= 4 ? load_word(abase, q - 4, lo, hi) : 0;
    W[5] = load_word(abase, q + 16, lo, hi);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) u.w[k] = W[1 + k];
    // starts of encodings at the unit's bytes -2 .. 15, as bit (k + 2)
    uint32_t m1 = 0, m2 = 0, m3 = 0, nl = 0;
#pragma unroll
    for (uint32_t j = 2; j < 20; ++j) {   // j: byte index into W; the unit's byte k is j = k + 4
        const uint32_t t = __funnelshift_r(W[j >> 2], W[(j >> 2) + 1], 8 * (j & 3)) & 0xFFFFFFu;
        const uint32_t b0 = t & 0xFFu, t2 = t & 0xFFFFu;
        if (j >= 4) {
            m1 |= (uint32_t)((b0 - 9u <= 4u) || b0 == 0x20u) << (j - 2);
            nl |= (uint32_t)(b0 == 0x0Au) << (j - 4);
        }
        if (j >= 3) m2 |= (uint32_t)(t2 == 0x85C2u || t2 == 0xA0C2u) << (j - 2);   // U+0085, U+00A0
        m3 |= (uint32_t)space3(t) << (j - 2);
    }
    const uint32_t S = ((m1 | m2 | (m2 << 1) | m3 | (m3 << 1) | (m3 << 2)) >> 2) & 0xFFFFu;
    uint32_t vm = 0xFFFFu;
    if (q < lo) vm &= 0xFFFFu << (uint32_t)(lo - q);
    if (q + 16 > hi) vm &= q >= hi ? 0u : 0xFFFFu >> (uint32_t)(q + 16 - hi);
    u.vm = vm; u.ns = ~S & vm; u.nl = nl & vm;
    return u;
}

// kind of the first event of a mask pair: 0 a '\n', 1 a non-space byte, 2 no event
__device__ __forceinline__ uint32_t first_kind(uint64_t ns, uint64_t ev) { return ev ? ((ns & (ev & (0 - ev))) ? 1u : 0u) : 2u; }

// The kept bytes of a lane's unit.  wkind: WAVES words of LDS.  flag: the tile's carry (the answer for a run of spaces at the tile's
// end); open: this lane's bytes behind its last event belong to that run.  Holds a __syncthreads.
__device__ __forceinline__ uint32_t kept_mask(const Unit &u, uint32_t flag, uint32_t *wkind, bool &open) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t ev = u.ns | u.nl, kind = first_kind(u.ns, ev);
    const uint64_t nsb = __ballot(kind == 1), evb = __ballot(kind != 2);
    if (lane == 0) wkind[wid] = first_kind(nsb, evb);
    __syncthreads();
    const uint64_t m = lane == 63 ? 0ull : evb & (~0ull << (lane + 1));   // the lanes behind this one that have an event
    uint32_t f = first_kind(nsb, m);
    for (uint32_t w = wid + 1; w < WAVES && f == 2; ++w) f = wkind[w];
    open = f == 2;
    if (open) f = flag;
    uint32_t kept = 0, cur = f;
#pragma unroll
    for (int i = 15; i >= 0; --i) {   // from the unit's last byte down: the answer is that of the nearest event at or behind the byte
        if ((ev >> i) & 1u) cur = (u.ns >> i) & 1u;
        kept |= cur << i;
    }
    return kept & u.vm;
}

}  // namespace

__global__ __launch_bounds__(THREADS) void k_split_reduce(SplitArgs a) {
    __shared__ uint32_t wkind[WAVES], wsum[WAVES][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const Unit u = load_unit(a, (uint64_t)blockIdx.x * TILE + tid * 16);
    bool open;
    const uint32_t kept = kept_mask(u, 0, wkind, open);
    const uint32_t ev = u.ns | u.nl;
    const uint32_t behind = ev ? u.vm & ~((2u << (31 - __clz(ev))) - 1u) : u.vm;   // the unit's bytes behind its last event
    const uint32_t counts = wave_sum(__popc(kept) | ((uint32_t)__popc(u.nl) << 16));   // (a tile has 4096 bytes: 16 bits each)
    const uint32_t run = wave_sum(open ? __popc(behind) : 0u);
    if (lane == 0) { wsum[wid][0] = counts; wsum[wid][1] = run; }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, r = 0, kind = 2;
        for (uint32_t w = 0; w < WAVES; ++w) { c += wsum[w][0]; r += wsum[w][1]; if (kind == 2) kind = wkind[w]; }
        a.agg[blockIdx.x] = SplitTile{c >> 16, c & 0xFFFFu, r, kind};
    }
}

// (the pattern of k_lines_scan, kgpu_format.hip; the loops run over the tiles, CARRY_K consecutive ones per thread and round -- a round
// costs a trip to memory and three barriers: 64 MiB are 16384 tiles, two rounds per direction)
constexpr uint32_t CARRY_K = 8;
__global__ __launch_bounds__(1024) void k_split_carry(SplitArgs a) {
    __shared__ uint32_t wk[16], wsum[16][2], carry_s[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x, nw = nthr >> 6, n = a.ntiles;
    const uint32_t per_round = nthr * CARRY_K, rounds = (n + per_round - 1) / per_round;
    if (tid == 0) carry_s[0] = 0;   // behind the last tile the block ends: a run of spaces there is trimmed
    __syncthreads();
    // backwards: agg[t].w = the kind of the first event in the tiles behind t
    for (uint32_t c = rounds; c-- > 0;) {
        const uint32_t i0 = (c * nthr + tid) * CARRY_K;
        uint32_t k[CARRY_K], kind = 2;
#pragma unroll
        for (uint32_t j = 0; j < CARRY_K; ++j) k[j] = i0 + j < n ? a.agg[i0 + j].w : 2u;
#pragma unroll
        for (int j = CARRY_K - 1; j >= 0; --j) if (k[j] != 2) kind = k[j];   // the first event of the thread's tiles
        const uint64_t nsb = __ballot(kind == 1), evb = __ballot(kind != 2);
        if (lane == 0) wk[wid] = first_kind(nsb, evb);
        __syncthreads();
        const uint64_t m = lane == 63 ? 0ull : evb & (~0ull << (lane + 1));
        uint32_t f = first_kind(nsb, m);
        for (uint32_t w = wid + 1; w < nw && f == 2; ++w) f = wk[w];
        if (f == 2) f = carry_s[0];
#pragma unroll
        for (int j = CARRY_K - 1; j >= 0; --j) {
            if (i0 + j < n) a.agg[i0 + j].w = f;
            if (k[j] != 2) f = k[j];
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t g = 2;
            for (uint32_t w = 0; w < nw && g == 2; ++w) g = wk[w];
            if (g != 2) carry_s[0] = g;
        }
        __syncthreads();
    }
    // forwards: exclusive sums of newlines and kept bytes (each thread reads its tiles' entries -- whose flags it wrote above -- before it writes them)
    if (tid == 0) carry_s[0] = carry_s[1] = 0;
    __syncthreads();
    for (uint32_t c = 0; c < rounds; ++c) {
        const uint32_t i0 = (c * nthr + tid) * CARRY_K;
        uint32_t vn[CARRY_K], vk[CARRY_K], fl[CARRY_K], tn = 0, tk = 0;
#pragma unroll
        for (uint32_t j = 0; j < CARRY_K; ++j) {
            SplitTile t{0, 0, 0, 0};
            if (i0 + j < n) t = a.agg[i0 + j];
            vn[j] = t.x; vk[j] = t.y + (t.w ? t.z : 0u); fl[j] = t.w;
            tn += vn[j]; tk += vk[j];
        }
        const uint32_t sn = wave_incl_scan(tn, lane), sk = wave_incl_scan(tk, lane);
        if (lane == 63) { wsum[wid][0] = sn; wsum[wid][1] = sk; }
        __syncthreads();
        uint32_t on = carry_s[0], ok = carry_s[1];
        for (uint32_t w = 0; w < wid; ++w) { on += wsum[w][0]; ok += wsum[w][1]; }
        uint32_t en = on + sn - tn, ek = ok + sk - tk;
#pragma unroll
        for (uint32_t j = 0; j < CARRY_K; ++j) {
            if (i0 + j < n) a.agg[i0 + j] = SplitTile{en, ek, 0, fl[j]};
            en += vn[j]; ek += vk[j];
        }
        __syncthreads();
        if (tid == nthr - 1) { carry_s[0] = on + sn; carry_s[1] = ok + sk; }
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t newlines = carry_s[0], kept = carry_s[1];
        const bool open_line = a.len && a.in[a.len - 1] != '\n';   // a last line without its newline
        const uint64_t lines = (uint64_t)newlines + (open_line ? 1 : 0);
        a.agg[n] = SplitTile{newlines, kept, (uint32_t)lines, 0};   // (lines <= len < 2^32)
        if (lines + 1 <= a.off_cap) {
            a.offsets[0] = 0;
            if (open_line) a.offsets[lines] = kept;
        }
        __hip_atomic_store(&a.host_ctl[0], (unsigned long long)lines, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host_ctl[1], (unsigned long long)kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(THREADS) void k_split_apply(SplitArgs a) {
    __shared__ uint32_t wkind[WAVES], wsum[WAVES];
    __shared__ uint32_t stage[TILE / 4 + 4];   // the tile's kept bytes in order (+ a word the last unit's funnel shift may read)
    if ((uint64_t)a.agg[a.ntiles].z + 1 > a.off_cap) return;   // the host reports KGPU_ERR_CAPACITY with the line count
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const SplitTile before = a.agg[blockIdx.x];   // newlines and kept bytes in front of the tile, the tile's flag
    const Unit u = load_unit(a, (uint64_t)blockIdx.x * TILE + tid * 16);
    bool open;
    const uint32_t kept = kept_mask(u, before.w, wkind, open);
    const uint32_t mine = __popc(kept) | ((uint32_t)__popc(u.nl) << 16);
    const uint32_t incl = wave_incl_scan(mine, lane);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    uint32_t excl = incl - mine, total = 0;
    for (uint32_t w = 0; w < WAVES; ++w) { if (w < wid) excl += wsum[w]; total += wsum[w]; }
    const uint32_t ek = excl & 0xFFFFu, en = excl >> 16, K = total & 0xFFFFu;
    uint8_t *sb = (uint8_t *)stage;
    if (kept == 0xFFFFu && (ek & 3u) == 0) {   // (most units of a text keep every byte)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) stage[(ek >> 2) + k] = u.w[k];
    } else {
        uint32_t o = ek;
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b)
            if ((kept >> b) & 1u) sb[o++] = (uint8_t)(u.w[b >> 2] >> (8 * (b & 3)));
    }
    for (uint32_t m = u.nl; m; m &= m - 1) {   // the line that ends at this '\n' ends at the count of kept bytes in front of it
        const uint32_t below = (m & (0 - m)) - 1u;
        const uint64_t line = (uint64_t)before.x + en + __popc(u.nl & below);
        if (line + 1 < a.off_cap) a.offsets[line + 1] = (uint64_t)before.y + ek + __popc(kept & below);   // (always, unless the block changed under the launches)
    }
    __syncthreads();
    // stage[0 .. K) -> out[before.y ..): bytes up to the first 16-byte boundary of the address space, whole units, bytes again
    if ((uint64_t)before.y + K > a.len) return;   // (never, unless the block changed under the launches)
    uint8_t *dst = a.out + before.y;
    const uint32_t to_boundary = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u), head = to_boundary < K ? to_boundary : K;
    const uint32_t nfull = (K - head) / 16;
    if (tid < head) dst[tid] = sb[tid];
    for (uint32_t j = tid; j < nfull; j += THREADS) {
        const uint32_t s = head + 16 * j, wi = s >> 2, sh = 8 * (s & 3);
        uint32_t r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) r[k] = __funnelshift_r(stage[wi + k], stage[wi + k + 1], sh);
        *(uint4 *)(dst + s) = make_uint4(r[0], r[1], r[2], r[3]);
    }
    const uint32_t tail = head + 16 * nfull;
    if (tail + tid < K) dst[tail + tid] = sb[tail + tid];
}

int launch_split_lines(const SplitArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (a.ntiles) hipLaunchKernelGGL(k_split_reduce, dim3(a.ntiles), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_split_carry, dim3(1), dim3(a.ntiles > 256 * CARRY_K ? 1024 : 256), 0, st, a);
    if (a.ntiles) hipLaunchKernelGGL(k_split_apply, dim3(a.ntiles), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

uint32_t split_tiles(const uint8_t *d_in, uint64_t len) {
    return len ? (uint32_t)((((uint64_t)(uintptr_t)d_in & 15u) + len + TILE - 1) / TILE) : 0u;
}

}  // namespace kgpu
