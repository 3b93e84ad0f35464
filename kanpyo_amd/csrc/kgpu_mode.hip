// kanpyo_amd/csrc/kgpu_mode.hip -- the search / extended mode decode of a batch on the device (include/kanpyo_gpu.h, "search mode"; not an output of the
// reference), over kept lattices ("The kept-lattice protocol"; kgpu_lattice_dev.h is the view of one).  kgpu_mode_host.cpp states the rule on the
// host; both run the statements of kgpu_mode_core.h.
//
// Four launches on the context's stream:
//   k_mode_forward  the hot path, one workgroup of FWD_WAVES wavefronts per sentence.  First the workgroup decodes the sentence's characters once (slab A's
//                   cbyte gives every character's byte offset) and leaves the kanji in front of every character position as u32[C + 1] in arena memory (a
//                   sentence may have any length): a node is all-kanji iff count[end] - count[start] == L, so a penalty is a few scalar operations and no
//                   loop over the node's characters; every node's word cost + penalty is made there and then, all nodes side by side, and parked in the
//                   node's state word (with the span and the counts loaded per target inside the sweep the kernel measured 1.11 to 1.14 times
//                   k_nbest_forward at k = 1: DESIGN 4.24).  Then the sweep, position after position (nodes are numbered by start position, and a predecessor
//                   starts in front of its target): the nodes of one start position are independent and dealt among the wavefronts, ONE WAVEFRONT PER
//                   TARGET; the lanes run over the bucket slots of the target's predecessors, 64 per round, each loading its predecessor's dp and ITS
//                   connection cost straight from the matrix (the layout and the read pattern of k_nbest_forward); one wave_min_u64 of the keys (tot, j)
//                   where that kernel sorts.  A key holds the predecessor's node index, so the result does not depend on the order a bucket's slots were
//                   filled in.  The state (dp << 32 | pre) is u64[N], in ONE slab with the counts, which the kernel takes itself (lat_take_slab).
//   k_mode_count    per sentence the chain's records (extended mode: an Unknown node counts its characters) and dp of EOS
//   k_mode_scan     one workgroup: the counts scanned in place; [n] = the batch's records
//   k_mode_write    the records, one wavefront per sentence: nothing when the total exceeds the capacity.  The chain is met from its end; the characters
//                   of an Unknown node in extended mode are dealt among the lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_lattice_dev.h"
#include "kgpu_mode_core.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t FWD_WAVES = 4;   // wavefronts of a forward workgroup: one sentence's targets of one start position are dealt among them

// A sentence's kept lattice with what lies at LAT_OWN: state u64[N] (dp << 32 | pre), then the kanji counts u32[C + 1] (the passes behind the forward
// kernel read the state alone).
struct ModeLat : KeptLat { const uint64_t *state; };
__device__ __forceinline__ ModeLat mode_lat(const ModeArgs &a, uint64_t s) {
    ModeLat l{kept_lat(a.arena, a.desc, s), nullptr};
    if (l.valid) l.state = (const uint64_t *)(a.arena + l.own);
    return l;
}

// The chain from EOS along pre: visit(node) for every node on it but its head, EOS first -> the nodes visited.  Bounded by N: a chain's nodes descend.
template <class F>
__device__ __forceinline__ uint32_t walk_chain(const ModeLat &l, F &&visit) {
    uint32_t node = l.N - 1, len = 0;
    for (uint32_t pre; (pre = mode_state_pre(l.state[node])) != MODE_NO_PRE && pre < node && len < l.N; node = pre, ++len) visit(node);
    return len;
}

}  // namespace

__global__ __launch_bounds__(64 * FWD_WAVES) void k_mode_forward(ModeArgs a) {
    __shared__ unsigned long long slab_off;   // lat_take_slab's word
    __shared__ uint32_t wave_kanji[FWD_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6);
    const kgpu_mode_opts opts = a.opts;
    const bool counted = opts.mode != KGPU_MODE_NORMAL;   // (NORMAL: every penalty is 0 and nothing reads the counts)
    const BatchArgs arena = lat_arena_args(a.ctl, a.arena, a.arena_bytes);
    // (every branch around a barrier below is workgroup-uniform: it tests what lat_take_slab gave, or the options)
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const KeptLat l = kept_lat<true>(a.arena, a.desc, s);
        if (!l.valid) continue;   // invalid UTF-8, or the lattice itself did not fit: the status says which
        const uint64_t N = l.N;
        const uint32_t C = l.C;
        const uint64_t off = lat_take_slab(a.desc + LAT_DESC_WORDS * s, 8ull * N + 4ull * ((uint64_t)C + 1), N, MODE_MAX_NODES, &slab_off, arena, a.status + s);
        if (off == LAT_NO_SLAB) continue;
        uint64_t *state = (uint64_t *)(a.arena + off);
        uint32_t *kanji = (uint32_t *)(state + N);   // [p]: the kanji among the characters in front of position p
        const uint32_t *cbyte = l.cbyte, *nb = l.nb, *boff = l.boff;
        const uint4 *nodeA = l.nodeA, *bucket = l.bucket;
        const uint2 *nodeB = l.nodeB;
        if (counted) {
            const uint8_t *text = a.utf8 + bcast64(a.offsets[s]);
            uint32_t carry = 0;
            if (threadIdx.x == 0) kanji[0] = 0;
            for (uint32_t base = 0; base < C; base += 64 * FWD_WAVES) {
                const uint32_t i = base + threadIdx.x;
                const uint32_t incl = wave_incl_scan(i < C && mode_is_kanji(mode_code_point(text + cbyte[i])) ? 1u : 0u, lane);
                if (lane == 63) wave_kanji[wave] = incl;
                __syncthreads();
                uint32_t front = carry;
#pragma unroll
                for (uint32_t w = 0; w < FWD_WAVES; ++w) { const uint32_t v = wave_kanji[w]; front += w < wave ? v : 0; carry += v; }
                if (i < C) kanji[i + 1] = front + incl;
                __syncthreads();
            }
            // every node's word cost with its penalty, all nodes side by side, parked in the node's state word until the sweep replaces it: the sweep
            // then has ONE load per target where it would have two dependent ones (the node's span, then the two counts) in front of its candidates
            for (uint64_t t = 1 + threadIdx.x; t < N; t += 64 * FWD_WAVES) {
                const uint4 nd = nodeA[t];
                const uint2 se = nodeB[t];
                state[t] = (uint32_t)((int32_t)nd.y + mode_penalty(opts, nd.w == 0, se.y - se.x, kanji[se.y] - kanji[se.x]));
            }
        }
        if (threadIdx.x == 0) state[0] = mode_bos_state();
        __syncthreads();
        for (uint32_t q = 0; q <= C; ++q) {   // the nodes that start at q: independent of each other, their predecessors' states are final -- dealt among the wavefronts
            const uint32_t t0 = bcast32(nb[q]), t1 = bcast32(nb[q + 1]), p0 = bcast32(boff[q]), P = bcast32(boff[q + 1]) - p0;
            for (uint32_t t = t0 + wave; t < t1; t += FWD_WAVES) {
                const uint4 nd = nodeA[t];
                const int16_t *col = a.conn + (size_t)a.conn_rows * (nd.x & 0xFFFFu);
                const int32_t word = counted ? (int32_t)(uint32_t)state[t] : (int32_t)nd.y;   // (NORMAL: every penalty is 0)
                uint64_t best = MODE_NONE;
                for (uint32_t c = lane; c < P; c += 64) {
                    const uint4 e = bucket[p0 + c];
                    const uint64_t key = mode_candidate(mode_state_dp(state[e.z]), e.z, word, (int32_t)col[e.y]);
                    best = key < best ? key : best;
                }
                best = wave_min_u64(best);
                if (lane == 0) state[t] = mode_state(best);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(TPB) void k_mode_count(ModeArgs a) {
    for (uint64_t s = (uint64_t)blockIdx.x * TPB + threadIdx.x; s < a.n; s += (uint64_t)gridDim.x * TPB) {
        const ModeLat l = mode_lat(a, s);
        uint64_t records = 0;
        if (l.valid) walk_chain(l, [&](uint32_t t) { const uint2 se = l.nodeB[t]; records += mode_record_count(a.opts.mode, class_of((int32_t)l.nodeA[t].w), se.x, se.y); });
        a.sent_len[s] = records;
        a.costs[s] = l.valid ? mode_state_dp(l.state[l.N - 1]) : NBEST_INF;
    }
}

__global__ __launch_bounds__(TPB) void k_mode_scan(ModeArgs a) { wg_excl_scan64<TPB>(a.sent_len, a.n); }

__global__ __launch_bounds__(TPB) void k_mode_write(ModeArgs a) {
    if (a.sent_len[a.n] > a.token_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (TPB / 64);
    for (uint64_t s = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); s < a.n; s += waves) {
        const ModeLat l = mode_lat(a, s);
        if (!l.valid) continue;
        uint64_t at = a.sent_len[s + 1];   // the chain is met from its end; every lane walks it, the stores are dealt among the lanes
        const uint64_t lo = a.sent_len[s];
        walk_chain(l, [&](uint32_t t) {
            const int32_t sid = (int32_t)l.nodeA[t].w;
            const uint2 se = l.nodeB[t];
            const uint32_t cls = class_of(sid), cnt = mode_record_count(a.opts.mode, cls, se.x, se.y);
            if (at - lo < cnt) { at = lo; return; }   // (cannot be: k_mode_count walked the same chain)
            at -= cnt;
            if (cnt == 1) {
                if (lane == 0) a.tokens[at] = lat_record(l, t);
                return;
            }
            for (uint32_t c = se.x + lane; c < se.y; c += 64) a.tokens[at + (c - se.x)] = mode_char_record(-sid, c, l.cbyte[c], l.cbyte[c + 1]);
        });
    }
}

int launch_mode_measure(const ModeArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const unsigned groups = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(a.n, 4096));
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n + TPB - 1) / TPB, 1024));
    hipLaunchKernelGGL(k_mode_forward, dim3(groups), dim3(64 * FWD_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_mode_count, dim3(blocks), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_mode_scan, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_mode_write(const ModeArgs &a, void *stream) {
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n + TPB / 64 - 1) / (TPB / 64), 1024));
    hipLaunchKernelGGL(k_mode_write, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
