// kanpyo_amd/csrc/kgpu_sentence.hip -- lines cut into sentences (include/kanpyo_gpu.h, "sentences") in HBM, byte for byte what kgpu_split_sentences_host
// makes of them: both decide by kgpu_sentence_core.h.  Work is dealt by BYTES, as in kgpu_split.hip: a tile is TILE = 4096 bytes of the address space
// (256 lanes x one aligned 16-byte load) of the packed text, whatever lines lie in it -- a 1 MB line is 256 tiles, ten thousand empty lines inside one
// tile are 40 offsets per lane.  A tile finds the lines that start in it by binary search in `offsets` and marks their first bytes in an LDS bitmap;
// a class is looked up in a window that ends where the line ends (the bitmap says where), so an encoding never reaches across two lines.
//
// Position-parallel, per byte j of a line (kgpu_sentence_core.h):
//   v(j) = min(0, v(j - 1) - d(j)),  u(j) = min(0, u(j + 1) + d(j + 1))      d: +1 opener, -1 closer;  eff(j) = 0  <=>  v(j) == 0 or u(j) == 0
//   cand(j)   j is the last byte of a terminator and no terminator starts at j + 1 inside the line
//   B(j)      cand(j) and eff(j) = 0: a boundary lies behind byte j
//   pend(j)   a boundary lies in front of j with nothing but SPACE between, inside the line      -> a sentence starts at j when pend(j) and j is no SPACE
//   drop(j)   j is SPACE, pend(j), and the first byte behind j that is no SPACE comes before the line's end
// v and u are scans of x -> min(a, x + b) (SentFn), segmented by the lines: a forward and a backward one.  pend is a forward scan of {0, 1, keep},
// drop's look-ahead a backward one of {line end, text, nothing}, as kgpu_split.hip's.  Which terminators are boundaries depends on v and u at the tile's
// two ends, and the NUMBER of boundaries is no closed form of them, so the counts need a reduce of their own behind the depth carry.  Five launches on the
// context's stream, none waits for another workgroup:
//   k_sent_reduce_a  a workgroup per tile -> agg_a[t]: the tile's forward and backward SentFn; tile_lines: the tile's first lines, by the only two
//                    searches of a tile (a wavefront each, 64 probes a step)
//   k_sent_carry_a   one workgroup: v at every tile's entry (forward), u behind every tile (backward) -> carry_a[t].  1024 threads, consecutive
//                    tiles per thread (one each up to 4 MiB of text, two up to 8 MiB, ...), a scan over the threads' compositions in between
//   k_sent_reduce_b  a workgroup per tile, v and u known -> agg_b[t]: lines that start in the tile, sentence starts and dropped bytes that need nothing
//                    from outside, the run of SPACE at either end, the kind of its first event and of its last (for pend), characters since the last
//                    line start
//   k_sent_carry_b   one workgroup: pend at every tile's entry, the first event behind every tile, then the exclusive sums of sentences and kept
//                    bytes and the characters in front of the tile in its first line -> carry_b[t]; carry_b[ntiles] = the totals; out_offsets[S];
//                    the two counts published to the host's mapped words
//   k_sent_apply     a workgroup per tile: everything again with the carries, kept bytes compacted into LDS in order and stored as aligned
//                    16-byte units; out_offsets and the 16-byte record of every sentence that starts in the tile.  Nothing is stored when
//                    S > sent_cap.
// The text is read three times (the second and third time from L2 / Infinity Cache for CLI-sized batches), the kept bytes written once; offsets are
// read by the binary searches and once per line: about 4 bytes moved per input byte, plus 8 read and 24 written per sentence.
#include <hip/hip_runtime.h>

#include "kgpu_device.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TILE = 4096;          // bytes per workgroup: 256 lanes x 16
constexpr uint32_t THREADS = TILE / 16;
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t CARRY_THREADS = 1024;
constexpr uint32_t LS_WORDS = (TILE + 64) / 32;   // the bitmap of line starts: bit p + 32 for tile position p in [-32, TILE + 32)
constexpr int32_t CLAMP = -(1 << 20);             // a carried v or u below this stays below zero whatever a tile adds

using Fn = SentFn<int32_t>;
using Fn64 = SentFn<int64_t>;
__device__ __forceinline__ Fn fn_id() { return Fn{0, 1 << 28, 0u}; }
__device__ __forceinline__ Fn64 fn64_id() { return Fn64{0, 1ll << 60, 0u}; }

// ---- the things a workgroup scans: combine(a, b) is "a, then b" ----
struct Kind { uint32_t k; };     // 2: nothing here, keep what came before
struct Sum2 { uint64_t a, b; };
struct Seg { uint32_t cnt, fixed; };   // a count since the last line start
__device__ __forceinline__ Fn combine(const Fn &a, const Fn &b) { return sent_then(a, b); }
__device__ __forceinline__ Fn64 combine(const Fn64 &a, const Fn64 &b) { return sent_then(a, b); }
__device__ __forceinline__ Kind combine(const Kind &a, const Kind &b) { return Kind{b.k != 2u ? b.k : a.k}; }
__device__ __forceinline__ Sum2 combine(const Sum2 &a, const Sum2 &b) { return Sum2{a.a + b.a, a.b + b.b}; }
__device__ __forceinline__ Seg combine(const Seg &a, const Seg &b) { return b.fixed ? b : Seg{a.cnt + b.cnt, a.fixed}; }
__device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)src, 64); }
__device__ __forceinline__ uint64_t shfl(uint64_t v, uint32_t src) { return ((uint64_t)shfl((uint32_t)(v >> 32), src) << 32) | shfl((uint32_t)v, src); }
__device__ __forceinline__ Fn shfl(const Fn &f, uint32_t src) { return Fn{(int32_t)shfl((uint32_t)f.b, src), (int32_t)shfl((uint32_t)f.a, src), shfl(f.fixed, src)}; }
__device__ __forceinline__ Fn64 shfl(const Fn64 &f, uint32_t src) { return Fn64{(int64_t)shfl((uint64_t)f.b, src), (int64_t)shfl((uint64_t)f.a, src), shfl(f.fixed, src)}; }
__device__ __forceinline__ Kind shfl(const Kind &f, uint32_t src) { return Kind{shfl(f.k, src)}; }
__device__ __forceinline__ Sum2 shfl(const Sum2 &f, uint32_t src) { return Sum2{shfl(f.a, src), shfl(f.b, src)}; }
__device__ __forceinline__ Seg shfl(const Seg &f, uint32_t src) { return Seg{shfl(f.cnt, src), shfl(f.fixed, src)}; }

// Exclusive scan over the workgroup's NW * 64 threads in thread order (REV: from the last thread down); total: the combination of all.  wtot: NW
// entries of LDS that nothing else uses until the next barrier behind the call.  Holds a __syncthreads.
template <uint32_t NW, bool REV, class T>
__device__ __forceinline__ T block_excl_scan(const T &v, const T &ident, T *wtot, T &total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t ll = REV ? 63 - lane : lane, lw = REV ? NW - 1 - wid : wid;   // the place in scan order
    T incl = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const T o = shfl(incl, (REV ? lane + off : lane - off) & 63u);
        if (ll >= off) incl = combine(o, incl);
    }
    T prev = shfl(incl, (REV ? lane + 1 : lane - 1) & 63u);
    if (ll == 0) prev = ident;
    if (ll == 63) wtot[lw] = incl;
    __syncthreads();
    T pre = ident;
    total = ident;
    for (uint32_t w = 0; w < NW; ++w) {
        const T t = wtot[w];
        if (w < lw) pre = combine(pre, t);
        total = combine(total, t);
    }
    return combine(pre, prev);
}

// ---- where the text lies ----
// Positions are those of the address space, counted from the 16-byte boundary at or in front of the text's first byte: the text is [lo, hi).
struct Geo { const uint8_t *abase; const uint64_t *offsets; uint64_t *tile_lines; uint64_t n, off0, lo, hi; };
__device__ __forceinline__ Geo geometry(const SentArgs &a) {
    Geo g;
    g.offsets = a.offsets; g.tile_lines = a.tile_lines; g.n = a.n; g.off0 = a.offsets[0];
    const uint8_t *in = a.utf8 + g.off0;
    const uint64_t mis = (uint64_t)(uintptr_t)in & 15u;
    g.abase = in - mis; g.lo = mis; g.hi = mis + a.total;
    return g;
}
__device__ __forceinline__ uint64_t line_pos(const Geo &g, uint64_t i) {   // where line i starts (inside [lo, hi] whatever the offsets say)
    const uint64_t o = g.offsets[i], rel = o > g.off0 ? o - g.off0 : 0;
    return g.lo + (rel < g.hi - g.lo ? rel : g.hi - g.lo);
}
// The first line of [l, r) that starts at or behind position x; r: none.
__device__ __forceinline__ uint64_t first_line_at(const Geo &g, uint64_t x, uint64_t l, uint64_t r) {
    while (l < r) {
        const uint64_t m = l + (r - l) / 2;
        if (line_pos(g, m) >= x) r = m; else l = m + 1;
    }
    return l;
}
// ... of all lines, by one whole wavefront: 64 probes a step (65 536 lines: three dependent loads instead of sixteen).
__device__ __forceinline__ uint64_t wave_first_line_at(const Geo &g, uint64_t x) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t l = 0, r = g.n;
    while (l < r) {
        const uint64_t step = (r - l) / 64 + 1, i = l + (uint64_t)lane * step + (step - 1);   // the last line of the lane's share of [l, r)
        const uint64_t ge = __ballot(i >= r || line_pos(g, i) >= x);                           // (never empty: 64 shares reach past r)
        const uint64_t k = (uint64_t)__ffsll((long long)ge) - 1;                               // the first share that ends at or behind x holds the answer
        l += k * step;
        r = l + (step - 1) < r ? l + (step - 1) : r;
    }
    return l;
}
// The lines a tile owns (their sentences' records are its business): those that start in it; the last tile also owns those that start at the text's end.
// tile_lines[2 t] is the first line that starts at or behind the tile's position -2, [2 t + 1] the first it owns ([2 ntiles + 1]: n): k_sent_reduce_a
// finds them, the later launches read them.
__device__ __forceinline__ void owned_lines(const Geo &g, uint32_t t, uint64_t &first, uint64_t &end) {
    first = g.tile_lines[2 * (uint64_t)t + 1];
    end = g.tile_lines[2 * (uint64_t)t + 3];
}

// The bitmap of line starts around tile t: bit p + 32 for a line that starts at tile position p in [-2, TILE + 4), and for the text's end.
template <bool SEARCH>
__device__ __forceinline__ void mark_line_starts(const Geo &g, uint32_t t, uint32_t ntiles, uint32_t *lsbits, uint64_t *shared_first) {
    const uint32_t tid = threadIdx.x;
    const uint64_t tbase = (uint64_t)t * TILE, from = tbase >= 2 ? tbase - 2 : 0, to = tbase + TILE + 4;
    for (uint32_t k = tid; k < LS_WORDS; k += THREADS) lsbits[k] = 0;
    if (SEARCH) {
        if (tid < 64) {
            const uint64_t v = wave_first_line_at(g, from);
            if (tid == 0) { *shared_first = v; g.tile_lines[2 * (uint64_t)t] = v; }
        } else if (tid < 128) {
            const uint64_t v = t ? wave_first_line_at(g, tbase) : 0;
            if (tid == 64) g.tile_lines[2 * (uint64_t)t + 1] = v;
        } else if (tid == 128 && t == 0) {
            g.tile_lines[2 * (uint64_t)ntiles + 1] = g.n;
        }
    } else if (tid == 0) {
        *shared_first = g.tile_lines[2 * (uint64_t)t];
    }
    __syncthreads();
    for (uint64_t i = *shared_first + tid; i < g.n; i += THREADS) {
        const uint64_t p = line_pos(g, i);
        if (p >= to) break;
        const uint32_t bit = (uint32_t)(p + 32 - tbase);
        atomicOr(&lsbits[bit >> 5], 1u << (bit & 31));
    }
    if (tid == 0 && g.hi >= from && g.hi < to) {
        const uint32_t bit = (uint32_t)(g.hi + 32 - tbase);
        atomicOr(&lsbits[bit >> 5], 1u << (bit & 31));
    }
    __syncthreads();
}

// Four aligned bytes at position q (a multiple of 4), zero where the text has none.
__device__ __forceinline__ uint32_t load_word(const Geo &g, uint64_t q) {
    if (q >= g.lo && q + 4 <= g.hi) return *(const uint32_t *)(g.abase + q);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (q + b >= g.lo && q + b < g.hi) v |= (uint32_t)g.abase[q + b] << (8 * b);
    return v;
}

// One lane's 16 bytes.  w: the bytes.  Masks over them, bit k for byte k: vm inside the text; sp SPACE; nc no 10xxxxxx; cand (above).  ls, op, cl have a
// 17th bit for the byte behind the unit: a line starts there (or the text ends), an opener / a closer starts there.
struct Unit { uint32_t w[4], vm, sp, nc, cand, ls, op, cl; };

__device__ __forceinline__ Unit load_unit(const Geo &g, const SentRule &rule, const uint32_t *lsbits, uint32_t t) {
    const uint32_t tid = threadIdx.x;
    const uint64_t q = (uint64_t)t * TILE + tid * 16;
    Unit u;
    uint32_t W[7];   // bytes q - 4 .. q + 20: the unit and a word on each side (W[6]: what a funnel shift by 0 reads)
    if (q >= g.lo && q + 16 <= g.hi) {
        const uint4 v = *(const uint4 *)(g.abase + q);
        W[1] = v.x; W[2] = v.y; W[3] = v.z; W[4] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) W[1 + k] = load_word(g, q + 4 * k);
    }
    W[0] = q >= 4 ? load_word(g, q - 4) : 0;
    W[5] = load_word(g, q + 16);
    W[6] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) u.w[k] = W[1 + k];
    // line starts at the unit's positions -2 .. 19, as bit (p + 2)
    const uint32_t b0 = tid * 16 + 30;
    const uint64_t two = (uint64_t)lsbits[b0 >> 5] | ((uint64_t)lsbits[(b0 >> 5) + 1] << 32);
    const uint32_t lsw = (uint32_t)(two >> (b0 & 31)) & 0x3FFFFFu;
    // what starts at the unit's positions -3 .. 16, as bit (p + 3); a window ends where its line does
    uint32_t tstart = 0, tlast = 0, sp = 0, op = 0, cl = 0;
#pragma unroll
    for (int j = -3; j <= 16; ++j) {
        const uint32_t idx = (uint32_t)(j + 4);
        uint32_t w = __funnelshift_r(W[idx >> 2], W[(idx >> 2) + 1], 8 * (idx & 3));
        const uint32_t nl = (lsw >> (j + 3)) & 7u;   // a line starts at position j + 1, j + 2, j + 3
        w &= (nl & 1u) ? 0xFFu : (nl & 2u) ? 0xFFFFu : (nl & 4u) ? 0xFFFFFFu : 0xFFFFFFFFu;
        const uint32_t tl = sent_term_len(rule, w), sl = sent_space_len(w);
        const int32_t d = sent_bracket(w);
        if (tl) { tstart |= 1u << (j + 3); tlast |= 1u << (j + 2 + tl); }
        sp |= ((1u << sl) - 1u) << (j + 3);
        op |= (uint32_t)(d > 0) << (j + 3);
        cl |= (uint32_t)(d < 0) << (j + 3);
    }
    uint32_t vm = 0xFFFFu;
    if (q < g.lo) vm &= 0xFFFFu << (uint32_t)(g.lo - q);
    if (q + 16 > g.hi) vm &= q >= g.hi ? 0u : 0xFFFFu >> (uint32_t)(q + 16 - g.hi);
    const uint32_t ls_next = (lsw >> 3) & 0xFFFFu;   // a line starts (the text ends) behind byte k
    u.vm = vm;
    u.sp = (sp >> 3) & vm;
    u.cand = (tlast >> 3) & ~((tstart >> 4) & ~ls_next) & vm;
    u.ls = (lsw >> 2) & 0x1FFFFu;
    u.op = rule.no_brackets ? 0u : (op >> 3) & 0x1FFFFu;
    u.cl = rule.no_brackets ? 0u : (cl >> 3) & 0x1FFFFu;
    uint32_t nc = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) nc |= (uint32_t)(((W[1 + (k >> 2)] >> (8 * (k & 3))) & 0xC0u) != 0x80u) << k;
    u.nc = nc & vm;
    return u;
}

__device__ __forceinline__ int32_t delta_at(const Unit &u, uint32_t k) { return (int32_t)((u.op >> k) & 1u) - (int32_t)((u.cl >> k) & 1u); }
__device__ __forceinline__ Fn fwd_step(const Unit &u, uint32_t k) { return sent_fwd_step<int32_t>(delta_at(u, k), (u.ls >> k) & 1u); }
__device__ __forceinline__ Fn bwd_step(const Unit &u, uint32_t k) { return sent_bwd_step<int32_t>(delta_at(u, k + 1), (u.ls >> (k + 1)) & 1u); }
// The lane's 16 bytes as one function: v in front of the unit -> v at its last byte; u behind the unit -> u at its first byte.
__device__ __forceinline__ Fn lane_fwd(const Unit &u) {
    if (!((u.op | u.cl | u.ls) & 0xFFFFu)) return fn_id();
    Fn f = fn_id();
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) f = sent_then(f, fwd_step(u, k));
    return f;
}
__device__ __forceinline__ Fn lane_bwd(const Unit &u) {
    if (!((u.op | u.cl | u.ls) >> 1)) return fn_id();
    Fn f = fn_id();
#pragma unroll
    for (int k = 15; k >= 0; --k) f = sent_then(f, bwd_step(u, (uint32_t)k));
    return f;
}

struct DepthLds { Fn wf[WAVES], wb[WAVES]; };
// The bytes of the unit whose enclosing depth is 0.  v_in / u_in: the tile's carries.
__device__ __forceinline__ uint32_t depth_zero(const Unit &u, int32_t v_in, int32_t u_in, DepthLds &l) {
    Fn tot;
    const Fn pf = block_excl_scan<WAVES, false>(lane_fwd(u), fn_id(), l.wf, tot);
    const Fn pb = block_excl_scan<WAVES, true>(lane_bwd(u), fn_id(), l.wb, tot);
    int32_t v = sent_apply(pf, v_in), x = sent_apply(pb, u_in);
    uint32_t zero = 0;
    if (!((u.op | u.cl | u.ls) & 0x1FFFFu)) return (v == 0 || x == 0) ? 0xFFFFu : 0u;   // (most units of a text: nothing moves the depth)
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) { v = sent_apply(fwd_step(u, k), v); zero |= (uint32_t)(v == 0) << k; }
#pragma unroll
    for (int k = 15; k >= 0; --k) { x = sent_apply(bwd_step(u, (uint32_t)k), x); zero |= (uint32_t)(x == 0) << k; }
    return zero;
}

// What becomes of the unit's bytes.  ns: a sentence starts (behind a boundary); drop: SPACE between two sentences; pend: as above.
// k_before: the pend scan's answer for the lanes in front (2: they are SPACE of one line all through); k_behind: the kind of the first event in the lanes
// behind (0 a line's end, 1 text, 2 none); first / last: the same two for the whole tile.
struct Fate { uint32_t ns, drop, pend, ev, k_before, k_behind, first, last; };
struct FateLds { Kind wp[WAVES], we[WAVES]; };
__device__ __forceinline__ Fate fate(const Unit &u, uint32_t boundary, uint32_t pend_in, uint32_t behind, FateLds &l) {
    Fate f;
    const uint32_t ls = u.ls & 0xFFFFu;
    // pend, forwards: raw(k + 1) = B(k) or (sp(k) and pend(k)), pend(k) = raw(k) and no line starts at k
    uint32_t out = 2;
    if (u.sp != 0xFFFFu || ls) {
        uint32_t raw = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t p = raw & ~(ls >> k) & 1u;
            raw = ((boundary >> k) | ((u.sp >> k) & p)) & 1u;
        }
        out = raw;
    }
    Kind tot;
    f.k_before = block_excl_scan<WAVES, false>(Kind{out}, Kind{2u}, l.wp, tot).k;
    f.last = tot.k;
    uint32_t raw = f.k_before == 2u ? pend_in : f.k_before, pend = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t p = raw & ~(ls >> k) & 1u;
        pend |= p << k;
        raw = ((boundary >> k) | ((u.sp >> k) & p)) & 1u;
    }
    f.pend = pend & u.vm;
    f.ns = f.pend & ~u.sp;
    // the first event behind each byte, backwards: an event is a byte that is no SPACE, or a line's first (the text's end is one)
    const uint32_t text = u.vm & ~u.sp & ~ls;
    f.ev = (u.vm & ~u.sp) | ls;
    const uint32_t mine = f.ev ? ((text & (f.ev & (0u - f.ev))) ? 1u : 0u) : 2u;
    f.k_behind = block_excl_scan<WAVES, true>(Kind{mine}, Kind{2u}, l.we, tot).k;
    f.first = tot.k;
    uint32_t cur = f.k_behind == 2u ? behind : f.k_behind, drop = 0;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        if ((f.ev >> k) & 1u) cur = (text >> k) & 1u;
        drop |= (uint32_t)(cur == 1u) << k;
    }
    f.drop = drop & u.sp & f.pend;
    return f;
}

}  // namespace

__global__ __launch_bounds__(THREADS) void k_sent_reduce_a(SentArgs a) {
    __shared__ uint32_t lsbits[LS_WORDS];
    __shared__ uint64_t first;
    __shared__ DepthLds dl;
    const Geo g = geometry(a);
    mark_line_starts<true>(g, blockIdx.x, a.ntiles, lsbits, &first);
    const Unit u = load_unit(g, a.rule, lsbits, blockIdx.x);
    Fn tf, tb;
    (void)block_excl_scan<WAVES, false>(lane_fwd(u), fn_id(), dl.wf, tf);
    (void)block_excl_scan<WAVES, true>(lane_bwd(u), fn_id(), dl.wb, tb);
    if (threadIdx.x == 0) a.agg_a[blockIdx.x] = SentAggA{tf.b, tf.a, tb.b, tb.a, tf.fixed | (tb.fixed << 1), 0u};
}

__global__ __launch_bounds__(CARRY_THREADS) void k_sent_carry_a(SentArgs a) {
    __shared__ Fn64 wtot[2][CARRY_THREADS / 64];
    const uint32_t tid = threadIdx.x, n = a.ntiles, per = (n + CARRY_THREADS - 1) / CARRY_THREADS;
    const uint32_t s = tid * per < n ? tid * per : n, e = s + per < n ? s + per : n;
    const auto fwd_of = [&](uint32_t t) { const SentAggA g = a.agg_a[t]; return Fn64{g.fb, g.fa, g.fixed & 1u}; };
    const auto bwd_of = [&](uint32_t t) { const SentAggA g = a.agg_a[t]; return Fn64{g.bb, g.ba, (g.fixed >> 1) & 1u}; };
    const auto clamped = [](int64_t x) { return (int32_t)(x < CLAMP ? CLAMP : x); };
    Fn64 f = fn64_id(), tot;
    for (uint32_t t = s; t < e; ++t) f = sent_then(f, fwd_of(t));
    int64_t x = sent_apply(block_excl_scan<CARRY_THREADS / 64, false>(f, fn64_id(), wtot[0], tot), (int64_t)0);
    for (uint32_t t = s; t < e; ++t) { a.carry_a[t].v_in = clamped(x); x = sent_apply(fwd_of(t), x); }
    f = fn64_id();
    for (uint32_t t = e; t-- > s;) f = sent_then(f, bwd_of(t));
    x = sent_apply(block_excl_scan<CARRY_THREADS / 64, true>(f, fn64_id(), wtot[1], tot), (int64_t)0);
    for (uint32_t t = e; t-- > s;) { a.carry_a[t].u_in = clamped(x); x = sent_apply(bwd_of(t), x); }
}

__global__ __launch_bounds__(THREADS) void k_sent_reduce_b(SentArgs a) {
    __shared__ uint32_t lsbits[LS_WORDS];
    __shared__ uint64_t first;
    __shared__ DepthLds dl;
    __shared__ FateLds fl;
    __shared__ Sum2 wsum[WAVES];
    __shared__ Seg wseg[WAVES];
    const uint32_t t = blockIdx.x;
    const Geo g = geometry(a);
    mark_line_starts<false>(g, t, a.ntiles, lsbits, &first);
    const Unit u = load_unit(g, a.rule, lsbits, t);
    const SentCarryA ca = a.carry_a[t];
    const uint32_t boundary = u.cand & depth_zero(u, ca.v_in, ca.u_in, dl);
    const Fate f = fate(u, boundary, 0, 0, fl);
    // the SPACE in front of the tile's first event, and the pending SPACE behind its last
    const uint32_t head = f.k_before == 2u ? __popc(u.vm & (f.ev ? (f.ev & (0u - f.ev)) - 1u : 0xFFFFu)) : 0u;
    const uint32_t tail = f.k_behind == 2u ? __popc(f.pend & (f.ev ? ~((2u << (31 - __clz(f.ev))) - 1u) : 0xFFFFu) & 0xFFFFu) : 0u;
    const uint32_t ls = u.ls & u.vm;
    const Seg mine{(uint32_t)__popc(ls ? u.nc & ~((1u << (31 - __clz(ls))) - 1u) : u.nc), ls ? 1u : 0u};
    Sum2 tot;
    Seg stot;
    (void)block_excl_scan<WAVES, false>(Sum2{(uint64_t)__popc(f.ns) | ((uint64_t)__popc(f.drop) << 32), (uint64_t)head | ((uint64_t)tail << 32)}, Sum2{0, 0}, wsum, tot);
    (void)block_excl_scan<WAVES, false>(mine, Seg{0, 0}, wseg, stot);
    if (threadIdx.x == 0) {
        uint64_t lf, le;
        owned_lines(g, t, lf, le);
        a.agg_b[t] = SentAggB{le - lf, (uint32_t)tot.a, (uint32_t)(tot.a >> 32), (uint32_t)tot.b, (uint32_t)(tot.b >> 32), f.first | (f.last << 2) | (stot.fixed << 4), stot.cnt};
    }
}

__global__ __launch_bounds__(CARRY_THREADS) void k_sent_carry_b(SentArgs a) {
    constexpr uint32_t NW = CARRY_THREADS / 64;
    __shared__ Kind wk[2][NW];
    __shared__ Sum2 wsum[NW];
    __shared__ Seg wseg[NW];
    const uint32_t tid = threadIdx.x, n = a.ntiles, per = (n + CARRY_THREADS - 1) / CARRY_THREADS;
    const uint32_t s = tid * per < n ? tid * per : n, e = s + per < n ? s + per : n;
    const Geo g = geometry(a);
    // pend at every tile's entry (forwards), the first event behind every tile (backwards; behind the last tile the text ends)
    Kind k{2u}, ktot;
    for (uint32_t t = s; t < e; ++t) k = combine(k, Kind{(a.agg_b[t].kinds >> 2) & 3u});
    k = block_excl_scan<NW, false>(k, Kind{2u}, wk[0], ktot);
    uint32_t cur = k.k == 2u ? 0u : k.k;
    for (uint32_t t = s; t < e; ++t) {
        a.carry_b[t].fl = cur;
        const uint32_t last = (a.agg_b[t].kinds >> 2) & 3u;
        if (last != 2u) cur = last;
    }
    k = Kind{2u};
    for (uint32_t t = e; t-- > s;) k = combine(k, Kind{a.agg_b[t].kinds & 3u});
    k = block_excl_scan<NW, true>(k, Kind{2u}, wk[1], ktot);
    cur = k.k == 2u ? 0u : k.k;
    for (uint32_t t = e; t-- > s;) {
        a.carry_b[t].fl |= cur << 1;
        const uint32_t first = a.agg_b[t].kinds & 3u;
        if (first != 2u) cur = first;
    }
    // each tile's sentences and kept bytes, then their exclusive sums; the characters in front of a tile in its first line
    const auto counts = [&](uint32_t t) {
        const SentAggB b = a.agg_b[t];
        const uint32_t fl = a.carry_b[t].fl, pend_in = fl & 1u, behind = fl >> 1, first = b.kinds & 3u;
        const uint64_t tlo = (uint64_t)t * TILE, thi = tlo + TILE;
        const uint64_t lo = tlo > g.lo ? tlo : g.lo, hi = thi < g.hi ? thi : g.hi, valid = hi > lo ? hi - lo : 0;
        const uint32_t ns = b.ns + ((pend_in && first == 1u) ? 1u : 0u);
        const uint32_t drop = b.dropped + ((pend_in && (first == 2u ? behind : first) == 1u) ? b.head : 0u) + ((first != 2u && behind == 1u) ? b.tail : 0u);
        return Sum2{b.lines + ns, valid - drop};
    };
    Sum2 sum{0, 0}, stot;
    Seg seg{0, 0}, segtot;
    for (uint32_t t = s; t < e; ++t) { sum = combine(sum, counts(t)); seg = combine(seg, Seg{a.agg_b[t].nc, (a.agg_b[t].kinds >> 4) & 1u}); }
    sum = block_excl_scan<NW, false>(sum, Sum2{0, 0}, wsum, stot);
    seg = block_excl_scan<NW, false>(seg, Seg{0, 0}, wseg, segtot);
    for (uint32_t t = s; t < e; ++t) {
        const Sum2 c = counts(t);
        const SentAggB b = a.agg_b[t];
        a.carry_b[t] = SentCarryB{sum.a, (uint32_t)sum.b, seg.cnt, a.carry_b[t].fl, 0u};
        sum = combine(sum, c);
        seg = combine(seg, Seg{b.nc, (b.kinds >> 4) & 1u});
    }
    if (tid == 0) {
        a.carry_b[n] = SentCarryB{stot.a, (uint32_t)stot.b, 0u, 0u, 0u};
        if (stot.a <= a.sent_cap) a.out_offsets[stot.a] = stot.b;
        __hip_atomic_store(&a.host_ctl[0], (unsigned long long)stot.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host_ctl[1], (unsigned long long)stot.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(THREADS) void k_sent_apply(SentArgs a) {
    __shared__ uint32_t lsbits[LS_WORDS];
    __shared__ uint64_t first;
    __shared__ DepthLds dl;
    __shared__ FateLds fl;
    __shared__ Sum2 wsum[WAVES];
    __shared__ uint32_t stage[TILE / 4 + 4];   // the tile's kept bytes in order (+ a word the last unit's funnel shift may read)
    __shared__ uint32_t lane_cnt[THREADS], lane_nc[THREADS], lane_m0[THREADS], lane_m1[THREADS];   // per lane: kept | ns << 16 and characters in front of it in the tile; its masks
    __shared__ uint64_t owned[2];
    const uint64_t S = a.carry_b[a.ntiles].sent_before;
    if (S > a.sent_cap) return;   // the host reports KGPU_ERR_CAPACITY with the count
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const Geo g = geometry(a);
    mark_line_starts<false>(g, t, a.ntiles, lsbits, &first);
    const Unit u = load_unit(g, a.rule, lsbits, t);
    const SentCarryA ca = a.carry_a[t];
    const SentCarryB cb = a.carry_b[t];
    const uint32_t boundary = u.cand & depth_zero(u, ca.v_in, ca.u_in, dl);
    const Fate f = fate(u, boundary, cb.fl & 1u, cb.fl >> 1, fl);
    const uint32_t kept = u.vm & ~f.drop;
    Sum2 tot;
    const Sum2 ex = block_excl_scan<WAVES, false>(Sum2{(uint64_t)__popc(kept) | ((uint64_t)__popc(f.ns) << 32), (uint64_t)__popc(u.nc)}, Sum2{0, 0}, wsum, tot);
    const uint32_t ek = (uint32_t)ex.a, K = (uint32_t)tot.a, NS = (uint32_t)(tot.a >> 32);
    lane_cnt[tid] = ek | ((uint32_t)(ex.a >> 32) << 16);
    lane_nc[tid] = (uint32_t)ex.b;
    lane_m0[tid] = kept | (f.ns << 16);
    lane_m1[tid] = u.nc;
    if (tid == 0) owned_lines(g, t, owned[0], owned[1]);
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
    __syncthreads();
    const uint64_t tbase = (uint64_t)t * TILE;
    // kept bytes, sentence starts and characters of the tile in front of its position p (<= TILE)
    const auto ranks = [&](uint32_t p, uint32_t &rk, uint32_t &rs, uint32_t &rc) {
        if (p >= TILE) { rk = K; rs = NS; rc = 0; return; }
        const uint32_t l = p >> 4, below = (1u << (p & 15)) - 1u, c = lane_cnt[l], m = lane_m0[l];
        rk = (c & 0xFFFFu) + __popc(m & below);
        rs = (c >> 16) + __popc((m >> 16) & below);
        rc = lane_nc[l] + __popc(lane_m1[l] & below);
    };
    const auto store = [&](uint64_t idx, uint64_t off, uint64_t line, uint32_t byte_start, uint32_t char_start) {
        if (idx >= a.sent_cap) return;   // (never, unless the text changed under the launches)
        a.out_offsets[idx] = off;
        *(uint4 *)(a.sents + idx) = make_uint4((uint32_t)line, (uint32_t)(line >> 32), byte_start, char_start);
    };
    // the first sentence of every line the tile owns
    for (uint64_t i = owned[0] + tid; i < owned[1]; i += THREADS) {
        const uint64_t p = line_pos(g, i) - tbase;
        uint32_t rk, rs, rc;
        ranks(p < TILE ? (uint32_t)p : TILE, rk, rs, rc);
        store(cb.sent_before + (i - owned[0]) + rs, (uint64_t)cb.kept_before + rk, i, 0u, 0u);
    }
    // the sentences that start behind a boundary
    for (uint32_t m = f.ns; m; m &= m - 1) {
        const uint32_t k = __ffs(m) - 1, p = tid * 16 + k;
        const uint64_t pos = tbase + p;
        const uint64_t line = first_line_at(g, pos + 1, owned[0], owned[1]) - 1;   // the last line that starts at or in front of the byte: an owned one, or the one in front of them
        const uint64_t lpos = line_pos(g, line);
        uint32_t rk, rs, rc, lk, lsn, lc;
        ranks(p, rk, rs, rc);
        uint32_t chars = cb.char_in + rc;
        if (lpos >= tbase) { ranks((uint32_t)(lpos - tbase), lk, lsn, lc); chars = rc - lc; }
        const uint64_t lines_upto = line + 1 > owned[0] ? line + 1 - owned[0] : 0;   // the owned lines that start at or in front of the byte
        store(cb.sent_before + lines_upto + rs, (uint64_t)cb.kept_before + rk, line, (uint32_t)(pos - lpos), chars);
    }
    // stage[0 .. K) -> out[kept_before ..): bytes up to the first 16-byte boundary of the address space, whole units, bytes again
    if ((uint64_t)cb.kept_before + K > a.total) return;   // (never, unless the text changed under the launches)
    uint8_t *dst = a.out + cb.kept_before;
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

uint32_t sent_tiles(uint64_t total) { return (uint32_t)((15u + total + TILE - 1) / TILE); }   // (whatever the text's alignment; one at least)

void sent_place_scratch(SentArgs &a, void *scratch) {
    const size_t m = (size_t)a.ntiles + 1;
    a.agg_b = (SentAggB *)scratch;
    a.carry_b = (SentCarryB *)(a.agg_b + m);
    a.agg_a = (SentAggA *)(a.carry_b + m);
    a.carry_a = (SentCarryA *)(a.agg_a + m);
    a.tile_lines = (uint64_t *)(a.carry_a + m);
}

int launch_split_sentences(const SentArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sent_reduce_a, dim3(a.ntiles), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sent_carry_a, dim3(1), dim3(CARRY_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sent_reduce_b, dim3(a.ntiles), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sent_carry_b, dim3(1), dim3(CARRY_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_sent_apply, dim3(a.ntiles), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
