// kanpyo_amd/csrc/kgpu_nbest.hip -- the N-best paths of a batch on the device (include/kanpyo_gpu.h, "N-best paths"; not an output of the reference:
// what `mecab -N k` prints), over kept lattices ("The kept-lattice protocol"; kgpu_lattice_dev.h is the view of one).  kgpu_nbest_host.cpp states
// the rule on the host; both run the statements of kgpu_nbest_core.h.
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
//                    The lists are u64[N][k] in a slab the kernel takes itself (lat_take_slab).
//   k_nbest_count    per (sentence, rank) the chain's length, per sentence its paths
//   k_nbest_scan     one workgroup: both arrays scanned in place; [n k] = the batch's records, [n] = its paths
//   k_nbest_write    the offsets, the costs and the records: nothing when the totals exceed the capacities
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_lattice_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t FWD_WAVES = 4;   // wavefronts of a forward workgroup: one sentence's targets of one start position are dealt among them

// A sentence's kept lattice with what lies at LAT_OWN: its lists, u64[N][k] (the passes behind the forward kernel).
struct ListLat : KeptLat { uint64_t *lists; };
__device__ __forceinline__ ListLat list_lat(const NbestArgs &a, uint64_t s) {
    ListLat l{kept_lat(a.arena, a.desc, s), nullptr};
    if (l.valid) l.lists = (uint64_t *)(a.arena + l.own);
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
__device__ __forceinline__ uint32_t walk_chain(const ListLat &l, uint32_t k, uint32_t rank, F &&visit) {
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
    __shared__ unsigned long long lists_off;   // lat_take_slab's word
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6), k = a.k;
    const BatchArgs arena = lat_arena_args(a.ctl, a.arena, a.arena_bytes);
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const KeptLat l = kept_lat<true>(a.arena, a.desc, s);
        if (!l.valid) continue;   // invalid UTF-8, or the lattice itself did not fit: the status says which
        const uint64_t off = lat_take_slab(a.desc + LAT_DESC_WORDS * s, 8ull * k * l.N, l.N, NBEST_MAX_NODES, &lists_off, arena, a.status + s);
        if (off == LAT_NO_SLAB) continue;
        uint64_t *lists = (uint64_t *)(a.arena + off);
        const uint32_t *nb = l.nb, *boff = l.boff;
        const uint4 *nodeA = l.nodeA, *bucket = l.bucket;
        const uint32_t C = l.C;
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
        const ListLat l = list_lat(a, s);
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
        const ListLat l = list_lat(a, s);
        const uint64_t p = a.path_offsets[s] + r;
        a.tok_offsets[p] = a.path_len[i];
        a.costs[p] = nbest_key_cost(l.lists[(uint64_t)(l.N - 1) * a.k + r]);
        kgpu_token *at = a.tokens + a.path_len[i + 1];   // the chain is met from its end
        walk_chain(l, a.k, r, [&](uint32_t t) { *--at = lat_record(l, t); });
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
