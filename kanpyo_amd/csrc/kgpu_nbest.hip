// kanpyo_amd/csrc/kgpu_nbest.hip -- the N-best paths of a batch on the device (include/kanpyo_gpu.h, "N-best paths"; not an output of the reference:
// what `mecab -N k` prints), over the lattices the general kernel left in the arena (BatchArgs::keep_lattice).  kgpu_nbest_host.cpp states the rule on the
// host; both run the statements of kgpu_nbest_core.h.
//
// Four launches on the context's stream:
//   k_nbest_forward  the hot path, one workgroup of FWD_WAVES wavefronts per sentence: every node's ranked list of k entries, position after position (nodes
//                    are numbered by start position, and a predecessor starts in front of its target); the nodes of one start position are independent
//                    and dealt among the wavefronts, ONE WAVEFRONT PER TARGET (one wavefront per sentence measured 2.4 to 3.4 times slower: DESIGN 4.22).
//                    For a target the lanes hold candidates (predecessor slot, rank), 64 per round: each
//                    lane loads its predecessor's key from that node's list and ITS connection cost straight from the matrix.  The 64 candidates are sorted
//                    in registers as 64-bit keys -- a bitonic network over the lanes, no LDS -- and merged with the running sorted top 64 of the rounds
//                    before: the elementwise minimum of A[i] and B[63 - i], then the six merge steps.  Lanes 0 .. k - 1 store the list.  A key holds the
//                    predecessor's node index and rank, so the result does not depend on the order a bucket's slots were filled in.
//                    The lists are u64[N][k] in a slab the kernel takes itself (slab_fresh: the arena cursor carries on behind the lattice launch).
//   k_nbest_count    per (sentence, rank) the chain's length, per sentence its paths
//   k_nbest_scan     one workgroup: both arrays scanned in place; [n k] = the batch's records, [n] = its paths
//   k_nbest_write    the offsets, the costs and the records: nothing when the totals exceed the capacities
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_device.h"
#include "kgpu_nbest_core.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t FWD_WAVES = 4;   // wavefronts of a forward workgroup: one sentence's targets of one start position are dealt among them

// One sentence's kept lattice (kgpu_internal.h: the slabs of k_tokenize_general) as the passes behind the forward kernel read it, and its lists.
struct Lat {
    bool valid;
    uint32_t N;
    const uint32_t *cbyte;
    const uint4 *nodeA; const uint2 *nodeB;
    uint64_t *lists;
};
__device__ __forceinline__ Lat lat_of(const NbestArgs &a, uint64_t s) {
    Lat l{};
    const unsigned long long *ds = a.desc + LAT_DESC_WORDS * s;
    l.valid = ds[5] != 0;
    if (!l.valid) return l;
    l.N = (uint32_t)ds[4];
    l.cbyte = (const uint32_t *)(a.arena + ds[0]) + SLAB_A_CBYTE * (ds[2] + 4);
    const uint8_t *sn = a.arena + ds[1];
    l.nodeA = (const uint4 *)sn; l.nodeB = (const uint2 *)(sn + (uint64_t)l.N * 32);
    l.lists = (uint64_t *)(a.arena + ds[7]);
    return l;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}
// Ascending sort of the wavefront's 64 keys, one per lane: the bitonic network, 21 compare-exchange steps.  Exec must be full.  cnt (wave-uniform): the
// lanes from cnt on hold NBEST_NONE, the largest key -- the stages that merge blocks of more than cnt / 2 lanes have nothing to move and are left out (a
// target of a few candidates, most of them at small k: 6 steps for 8 candidates).
__device__ __forceinline__ uint64_t wave_sort64(uint64_t v, uint32_t lane, uint32_t cnt) {
#pragma unroll
    for (uint32_t sz = 2; sz <= 64; sz <<= 1) {
        if (cnt <= sz / 2) break;
#pragma unroll
        for (uint32_t d = sz >> 1; d > 0; d >>= 1) {
            const uint64_t o = shfl64(v, lane ^ d);
            const bool keep_min = ((lane & d) == 0) == ((lane & sz) == 0);
            v = (o < v) == keep_min ? o : v;
        }
    }
    return v;
}
// The 64 smallest of two ascending runs, ascending: min(A[i], B[63 - i]) is bitonic and holds them; six half-cleaners sort it.
__device__ __forceinline__ uint64_t wave_merge64(uint64_t a, uint64_t b, uint32_t lane) {
    const uint64_t br = shfl64(b, 63u - lane);
    uint64_t v = br < a ? br : a;
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const uint64_t o = shfl64(v, lane ^ d);
        v = (o < v) == ((lane & d) == 0) ? o : v;
    }
    return v;
}

// The chain of path (node, rank) down to BOS: visit(node) for every node on it, EOS first -> the nodes visited.  Bounded by N: a chain's nodes descend.
template <class F>
__device__ __forceinline__ uint32_t walk_chain(const Lat &l, uint32_t k, uint32_t rank, F &&visit) {
    uint32_t node = l.N - 1, len = 0;
    while (node != 0 && len < l.N) {
        visit(node);
        const uint64_t key = l.lists[(uint64_t)node * k + rank];
        node = nbest_key_pred(key); rank = nbest_key_rank(key);
        ++len;
    }
    return len;
}

}  // namespace

__global__ __launch_bounds__(64 * FWD_WAVES) void k_nbest_forward(NbestArgs a) {
    __shared__ unsigned long long lists_off;   // the arena offset of the sentence's lists (~0: they did not fit), from wavefront 0 to the others
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6), k = a.k;
    BatchArgs arena{};   // (what slab_fresh reads)
    arena.ctl = a.ctl; arena.arena = a.arena; arena.arena_bytes = a.arena_bytes;
    // (every branch around a barrier below is workgroup-uniform: it tests the sentence's descriptor, which only this workgroup writes, or lists_off)
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        unsigned long long *ds = a.desc + LAT_DESC_WORDS * s;
        if (bcast32((uint32_t)ds[5]) == 0) continue;   // invalid UTF-8, or the lattice itself did not fit: the status says which
        const uint64_t N = bcast64(ds[4]);
        if (wave == 0) {
            Slab sl{nullptr, 0};
            const bool ok = N < NBEST_MAX_NODES && slab_fresh(sl, 8ull * k * N, arena, lane);
            if (lane == 0) lists_off = ok ? (unsigned long long)(sl.ptr - a.arena) : ~0ull;
        }
        __syncthreads();
        const uint64_t off = bcast64(lists_off);
        __syncthreads();   // (read by all before the next sentence's is stored)
        if (off == ~0ull) {
            if (threadIdx.x == 0) { a.status[s] = KGPU_SENT_NO_SCRATCH; ds[5] = 0; }
            continue;
        }
        if (threadIdx.x == 0) ds[7] = off;
        uint64_t *lists = (uint64_t *)(a.arena + off);
        const uint32_t *sa = (const uint32_t *)(a.arena + ds[0]);
        const uint64_t na = bcast64(ds[2]) + 4;
        const uint32_t *nb = sa + SLAB_A_NB * na, *boff = sa + SLAB_A_BOFF * na;
        const uint8_t *sn = a.arena + ds[1];
        const uint4 *nodeA = (const uint4 *)sn, *bucket = (const uint4 *)(sn + N * 16);
        const uint32_t C = bcast32((uint32_t)ds[3]);
        if (threadIdx.x < k) lists[threadIdx.x] = threadIdx.x == 0 ? nbest_bos_key() : NBEST_NONE;   // L(BOS)
        __syncthreads();
        for (uint32_t q = 0; q <= C; ++q) {   // the nodes that start at q: independent of each other, their predecessors' lists are final -- dealt among the wavefronts
            const uint32_t t0 = bcast32(nb[q]), t1 = bcast32(nb[q + 1]), p0 = bcast32(boff[q]), P = bcast32(boff[q + 1]) - p0;
            const uint64_t total = (uint64_t)P * k;
            for (uint32_t t = t0 + wave; t < t1; t += FWD_WAVES) {
                const uint4 nd = nodeA[t];
                const int16_t *col = a.conn + (size_t)a.conn_rows * (nd.x & 0xFFFFu);
                uint64_t top = NBEST_NONE;
                for (uint64_t c0 = 0; c0 < total; c0 += 64) {
                    const uint64_t c = c0 + lane;
                    uint64_t key = NBEST_NONE;
                    if (c < total) {
                        const uint32_t slot = (uint32_t)(c / k), r = (uint32_t)(c - (uint64_t)slot * k);
                        const uint4 e = bucket[p0 + slot];
                        key = nbest_candidate(lists[(uint64_t)e.z * k + r], e.z, r, (int32_t)nd.y, (int32_t)col[e.y]);
                    }
                    key = wave_sort64(key, lane, (uint32_t)min((uint64_t)64, total - c0));
                    top = c0 ? wave_merge64(top, key, lane) : key;
                }
                if (lane < k) lists[(uint64_t)t * k + lane] = top;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(TPB) void k_nbest_count(NbestArgs a) {
    const uint64_t items = a.n * a.k;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < items; i += (uint64_t)gridDim.x * TPB) {
        const uint64_t s = i / a.k;
        const uint32_t r = (uint32_t)(i - s * a.k);
        const Lat l = lat_of(a, s);
        const uint64_t *eos = l.valid ? l.lists + (uint64_t)(l.N - 1) * a.k : nullptr;
        a.path_len[i] = l.valid && eos[r] != NBEST_NONE ? walk_chain(l, a.k, r, [](uint32_t) {}) : 0;
        if (r == 0) {
            uint32_t paths = 0;
            while (l.valid && paths < a.k && eos[paths] != NBEST_NONE) ++paths;
            a.path_offsets[s] = paths;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_nbest_scan(NbestArgs a) {
    wg_excl_scan64<TPB>(a.path_len, a.n * a.k);
    wg_excl_scan64<TPB>(a.path_offsets, a.n);
}

__global__ __launch_bounds__(TPB) void k_nbest_write(NbestArgs a) {
    const uint64_t items = a.n * a.k;
    if (a.path_len[items] > a.token_cap || a.path_offsets[a.n] > a.path_cap) return;   // the host reports KGPU_ERR_CAPACITY with the sizes needed
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tok_offsets[a.path_offsets[a.n]] = a.path_len[items];
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < items; i += (uint64_t)gridDim.x * TPB) {
        const uint64_t s = i / a.k;
        const uint32_t r = (uint32_t)(i - s * a.k);
        if (r >= a.path_offsets[s + 1] - a.path_offsets[s]) continue;
        const Lat l = lat_of(a, s);
        const uint64_t p = a.path_offsets[s] + r;
        a.tok_offsets[p] = a.path_len[i];
        a.costs[p] = nbest_key_cost(l.lists[(uint64_t)(l.N - 1) * a.k + r]);
        kgpu_token *at = a.tokens + a.path_len[i + 1];   // the chain is met from its end
        walk_chain(l, a.k, r, [&](uint32_t t) {
            const int32_t sid = (int32_t)l.nodeA[t].w;
            const uint2 se = l.nodeB[t];
            const uint32_t bs = l.cbyte[se.x];
            *--at = nbest_record(sid > 0 ? KGPU_CLASS_KNOWN : sid < 0 ? KGPU_CLASS_UNKNOWN : KGPU_CLASS_DUMMY, sid < 0 ? -sid : sid, bs, se.x, se.y, l.cbyte[se.y] - bs);
        });
    }
}

int launch_nbest_measure(const NbestArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const unsigned groups = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(a.n, 4096));
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n * a.k + TPB - 1) / TPB, 1024));
    hipLaunchKernelGGL(k_nbest_forward, dim3(groups), dim3(64 * FWD_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_nbest_count, dim3(blocks), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_nbest_scan, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_nbest_write(const NbestArgs &a, void *stream) {
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n * a.k + TPB - 1) / TPB, 1024));
    hipLaunchKernelGGL(k_nbest_write, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
