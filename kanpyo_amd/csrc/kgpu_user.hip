// kanpyo_amd/csrc/kgpu_user.hip -- the user dictionary over a batch on the device (include/kanpyo_gpu.h, "user dictionary"; not an output of the
// reference), over kept lattices ("The kept-lattice protocol"; kgpu_lattice_dev.h is the view of one).  kgpu_user_host.cpp states the rule on
// the host; both run the statements of kgpu_user_core.h and kgpu_mode_core.h.  Nothing of the kept lattice is changed: the user nodes lie beside it.
//
// Four launches on the context's stream:
//   k_user_forward  one workgroup of FWD_WAVES wavefronts per sentence, in three parts.
//                   MATCH: one lane per start character probes the table once per key length that exists (user_match: a hash probe, every hit confirmed
//                   by its bytes) and leaves the matches of its position in slab A's dead path[] array; a workgroup scan gives every position's first
//                   user node and U.  ONE slab (lat_take_slab; UserArgs has its layout) for N + U states, the kanji counts and the user nodes.
//                   LAY OUT: the lanes match again and write their positions' user nodes by entry (a group is in entry order; a node's rank is its
//                   place in its group plus the entries below it in the position's other groups, a binary search each), say whether the position's
//                   Unknown nodes are withdrawn, and count the user nodes per END position; a second scan and a scatter group them by end (a
//                   counting sort: fill order is free, a key carries the node's index).  Every node's word cost with its penalty is parked in its
//                   state word; a withdrawn node gets USER_WITHDRAWN there.  A handle without entries skips MATCH and LAY OUT.
//                   SWEEP: k_mode_forward's, position after position, one wavefront per target, the lanes over the predecessors 64 per round, each
//                   loading its predecessor's state and ITS connection cost, one wave_min_u64 of the keys (tot, j) -- with two ranges of targets
//                   (lattice, user) and two of predecessors (the bucket's slots, the end-sorted user nodes) at every position.
//   k_user_count    per sentence the chain's records and dp of EOS
//   k_user_scan     one workgroup: the counts scanned in place; [n] = the batch's records
//   k_user_write    the records, one wavefront per sentence: a lattice node's as k_mode_write has them, a user node's from the slab
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_lattice_dev.h"
#include "kgpu_user_core.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t FWD_WAVES = 4;   // wavefronts of a forward workgroup
constexpr uint32_t FWD_TPB = 64 * FWD_WAVES;

// The slab of a sentence with N nodes, C characters and U user nodes (UserArgs has the order).
struct UserSlab {
    uint32_t U;
    uint4 *unode;        // [U]: x = left id | right id << 16, y = the entry's cost, z, w = start and end character position
    uint64_t *state;     // [N + U]: dp << 32 | pre, the combined index
    uint32_t *kanji;     // [C + 1]
    uint32_t *ub;        // [C + 2]: the user nodes that START at q are [ub[q], ub[q + 1])
    uint32_t *ue_cnt;    // [C + 2]: the user nodes that END at p, counted
    uint32_t *ue_off;    // [C + 2]: ... their slots in ue_idx are [ue_off[p], ue_off[p + 1])
    uint32_t *ue_idx;    // [U]
    uint32_t *uent;      // [U]: the node's entry
};
__host__ __device__ constexpr uint64_t user_slab_bytes(uint64_t N, uint64_t C, uint64_t U) { return 8 * N + 32 * U + 16 * C + 44; }
__device__ __forceinline__ UserSlab user_slab(uint8_t *p, uint64_t N, uint64_t C, uint32_t U) {
    UserSlab s;
    s.U = U;
    s.unode = (uint4 *)(p + 16);
    s.state = (uint64_t *)(p + 16 + 16ull * U);
    s.kanji = (uint32_t *)(s.state + N + U);
    s.ub = s.kanji + C + 1;
    s.ue_cnt = s.ub + C + 2;
    s.ue_off = s.ue_cnt + C + 2;
    s.ue_idx = s.ue_off + C + 2;
    s.uent = s.ue_idx + U;
    return s;
}

// A sentence's kept lattice with its slab (the passes behind the forward kernel).
struct UserLat : KeptLat { UserSlab sl; };
__device__ __forceinline__ UserLat user_lat(const UserArgs &a, uint64_t s) {
    UserLat l{kept_lat(a.m.arena, a.m.desc, s), UserSlab{}};
    if (l.valid) l.sl = user_slab(a.m.arena + l.own, l.N, l.C, *(const uint32_t *)(a.m.arena + l.own));
    return l;
}

// The chain from EOS along pre over the combined indices: visit(node) for every node on it but its head, EOS first -> the nodes visited.  Bounded by
// N + U: a chain's nodes start in front of each other.
template <class F>
__device__ __forceinline__ uint32_t walk_chain(const UserLat &l, F &&visit) {
    const uint32_t total = l.N + l.sl.U;
    uint32_t node = l.N - 1, len = 0;
    for (uint32_t pre; (pre = mode_state_pre(l.sl.state[node])) != MODE_NO_PRE && pre < total && len < total; node = pre, ++len) visit(node);
    return len;
}
__device__ __forceinline__ uint32_t node_records(const UserLat &l, uint32_t mode, uint32_t t) {
    if (t >= l.N) return 1u;
    const uint2 se = l.nodeB[t];
    return mode_record_count(mode, class_of((int32_t)l.nodeA[t].w), se.x, se.y);
}

// Exclusive scan of in[0 .. n) into out[0 .. n) (the same array, or another) by the whole forward workgroup -> the total.  L2: the input was made by
// atomic adds, which the CU's L1 does not see.  Workgroup-uniform control flow; two barriers per round.
template <bool L2>
__device__ __forceinline__ uint64_t wg_scan32(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *wave_sum_lds) {
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6);
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += FWD_TPB) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n ? (L2 ? ld_l2(in + i) : in[i]) : 0u;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (lane == 63) wave_sum_lds[wave] = incl;
        __syncthreads();
        uint64_t front = carry;
#pragma unroll
        for (uint32_t w = 0; w < FWD_WAVES; ++w) { const uint32_t x = wave_sum_lds[w]; front += w < wave ? x : 0; carry += x; }
        if (i < n) out[i] = (uint32_t)(front + incl - v);
        __syncthreads();
    }
    return carry;
}

}  // namespace

__global__ __launch_bounds__(FWD_TPB) void k_user_forward(UserArgs ua) {
    __shared__ unsigned long long slab_off;   // lat_take_slab's word
    __shared__ uint32_t wave_part[FWD_WAVES];
    const ModeArgs &a = ua.m;
    const UserTableView tv = ua.t;
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6);
    const kgpu_mode_opts opts = a.opts;
    const bool counted = opts.mode != KGPU_MODE_NORMAL;   // (NORMAL: every penalty is 0 and nothing reads the counts)
    const bool any = tv.n_groups != 0;
    const BatchArgs arena = lat_arena_args(a.ctl, a.arena, a.arena_bytes);
    // (every branch around a barrier below is workgroup-uniform: it tests what lat_take_slab gave, the options, or whether the handle has entries)
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const KeptLat l = kept_lat<true>(a.arena, a.desc, s);
        if (!l.valid) continue;   // invalid UTF-8, or the lattice itself did not fit: the status says which
        const uint64_t N = l.N;
        const uint32_t C = l.C;
        const uint8_t *text = a.utf8 + bcast64(a.offsets[s]);
        const uint32_t *cbyte = l.cbyte, *nb = l.nb, *boff = l.boff;
        const uint4 *nodeA = l.nodeA, *bucket = l.bucket;
        const uint2 *nodeB = l.nodeB;
        uint32_t *path = l.path;   // [q < C]: first the matches at q, then the first user node of q, then whether q's Unknown nodes are withdrawn
        // ---- match: how many entries stand at every position (a handle without entries: none, and nothing of the match or the lay-out runs) ----
        uint64_t U64 = 0;
        if (any) {
            for (uint32_t q = threadIdx.x; q < C; q += FWD_TPB) path[q] = user_match(tv, text, cbyte, C, q, [](uint32_t, uint32_t) {});
            __syncthreads();
            U64 = wg_scan32<false>(path, path, C, wave_part);
        }
        const uint64_t off = lat_take_slab(a.desc + LAT_DESC_WORDS * s, user_slab_bytes(N, C, U64), N + U64, USER_MAX_NODES, &slab_off, arena, a.status + s);
        if (off == LAT_NO_SLAB) continue;
        const uint32_t U = (uint32_t)U64;
        const UserSlab sl = user_slab(a.arena + off, N, C, U);
        uint64_t *state = sl.state;
        uint32_t *kanji = sl.kanji;
        if (counted) {
            uint32_t carry = 0;
            if (threadIdx.x == 0) kanji[0] = 0;
            for (uint32_t base = 0; base < C; base += FWD_TPB) {
                const uint32_t i = base + threadIdx.x;
                const uint32_t incl = wave_incl_scan(i < C && mode_is_kanji(mode_code_point(text + cbyte[i])) ? 1u : 0u, lane);
                if (lane == 63) wave_part[wave] = incl;
                __syncthreads();
                uint32_t front = carry;
#pragma unroll
                for (uint32_t w = 0; w < FWD_WAVES; ++w) { const uint32_t v = wave_part[w]; front += w < wave ? v : 0; carry += v; }
                if (i < C) kanji[i + 1] = front + incl;
                __syncthreads();
            }
        }
        for (uint32_t p = threadIdx.x; p < C + 2; p += FWD_TPB) { sl.ue_cnt[p] = 0; sl.ue_off[p] = 0; sl.ub[p] = any && p < C ? path[p] : U; }
        if (threadIdx.x == 0) { *(uint32_t *)(a.arena + off) = U; state[0] = mode_bos_state(); }
        __syncthreads();
        // ---- lay out: a lane writes the user nodes of its position, by entry ----
        if (any) {
            for (uint32_t q = threadIdx.x; q < C; q += FWD_TPB) {
                const uint32_t base = sl.ub[q], n = sl.ub[q + 1] - base;
                uint32_t flag = 0;
                if (n) {
                    // the position's groups, shortest key first, wait in the state words of its own user nodes (a group has an entry at least: they fit)
                    uint32_t m = 0;
                    user_match(tv, text, cbyte, C, q, [&](uint32_t g, uint32_t L) {
                        if (m < n) state[N + base + m] = (uint64_t)g | ((uint64_t)L << 32);
                        ++m;
                    });
                    m = m < n ? m : n;
                    // a group is in entry order already: an entry's place among the position's nodes is its place in its group plus the entries below it
                    // in every other group -- a binary search each, linear in the position's matches where an insertion sort would be quadratic
                    for (uint32_t ga = 0; ga < m; ++ga) {
                        const uint64_t w = state[N + base + ga];
                        const UserGroup gr = tv.groups[(uint32_t)w];
                        const uint32_t end = q + (uint32_t)(w >> 32);
                        for (uint32_t i = 0; i < gr.count; ++i) {
                            const UserEntry en = tv.ents[gr.first + i];
                            uint32_t rank = i;
                            for (uint32_t gb = 0; gb < m; ++gb) {
                                if (gb == ga) continue;
                                const UserGroup other = tv.groups[(uint32_t)state[N + base + gb]];
                                rank += user_entries_below(tv.ents + other.first, other.count, en.entry);
                            }
                            if (rank < n) { sl.unode[base + rank] = uint4{en.ids, (uint32_t)en.cost, q, end}; sl.uent[base + rank] = en.entry; }
                        }
                    }
                    for (uint32_t i = 0; i < n; ++i) state[N + base + i] = atomicAdd(&sl.ue_cnt[sl.unode[base + i].w], 1u);   // its place among the nodes of its end
                    bool known = false;
                    for (uint32_t t = nb[q], t1 = nb[q + 1]; t < t1; ++t) known |= (int32_t)nodeA[t].w > 0;
                    const uint32_t cp = mode_code_point(text + cbyte[q]);
                    const uint32_t cat = ua.cat[cp < ua.cat_len ? cp : 0u];
                    flag = user_withdrawn(n, known, (ua.cinfo[cat].flags & CAT_INVOKE) != 0) ? 1u : 0u;
                }
                path[q] = flag;
            }
            __syncthreads();
            wg_scan32<true>(sl.ue_cnt, sl.ue_off, C + 2, wave_part);
        }
        // every lattice node's word cost with its penalty, parked in its state word until the sweep replaces it; a withdrawn node's stays what it is here
        for (uint64_t t = 1 + threadIdx.x; t < N; t += FWD_TPB) {
            const uint4 nd = nodeA[t];
            const uint2 se = nodeB[t];
            const bool gone = any && (int32_t)nd.w < 0 && se.x < C && path[se.x] != 0;
            state[t] = gone ? USER_WITHDRAWN : (uint64_t)(uint32_t)((int32_t)nd.y + mode_penalty(opts, nd.w == 0, se.y - se.x, counted ? kanji[se.y] - kanji[se.x] : 0u));
        }
        __syncthreads();
        // ... and every user node's, once the node has gone to its slot among those of its end
        for (uint32_t u = threadIdx.x; u < U; u += FWD_TPB) {
            const uint4 nd = sl.unode[u];
            sl.ue_idx[sl.ue_off[nd.w] + (uint32_t)state[N + u]] = u;
            state[N + u] = (uint32_t)((int32_t)nd.y + mode_penalty(opts, false, nd.w - nd.z, counted ? kanji[nd.w] - kanji[nd.z] : 0u));
        }
        __syncthreads();
        // ---- sweep: the nodes that start at q are independent of each other, their predecessors' states are final -- dealt among the wavefronts ----
        for (uint32_t q = 0; q <= C; ++q) {
            const uint32_t t0 = bcast32(nb[q]), T1 = bcast32(nb[q + 1]) - t0, u0 = bcast32(sl.ub[q]), T = T1 + (bcast32(sl.ub[q + 1]) - u0);
            const uint32_t p0 = bcast32(boff[q]), P1 = bcast32(boff[q + 1]) - p0, v0 = bcast32(sl.ue_off[q]), P = P1 + (bcast32(sl.ue_off[q + 1]) - v0);
            for (uint32_t i = wave; i < T; i += FWD_WAVES) {
                const bool lattice = i < T1;
                const uint32_t idx = lattice ? t0 + i : (uint32_t)N + u0 + (i - T1);
                const uint32_t ids = lattice ? nodeA[idx].x : sl.unode[idx - (uint32_t)N].x;
                const uint64_t parked = state[idx];   // (a withdrawn target runs the rounds too and stores nothing: a branch here would put this load's
                                                      // round trip in front of the predecessors' loads at every position, where it now lies beside them)
                const int16_t *col = a.conn + (size_t)a.conn_rows * (ids & 0xFFFFu);
                const int32_t word = (int32_t)(uint32_t)parked;
                uint64_t best = MODE_NONE;
                for (uint32_t c = lane; c < P; c += 64) {
                    uint32_t j, right;
                    if (c < P1) { const uint4 e = bucket[p0 + c]; j = e.z; right = e.y; }
                    else { const uint32_t u = sl.ue_idx[v0 + (c - P1)]; j = (uint32_t)N + u; right = sl.unode[u].x >> 16; }
                    const uint64_t sj = state[j];
                    const uint64_t key = sj == USER_WITHDRAWN ? MODE_NONE : mode_candidate(mode_state_dp(sj), j, word, (int32_t)col[right]);
                    best = key < best ? key : best;
                }
                best = wave_min_u64(best);
                if (lane == 0 && parked != USER_WITHDRAWN) state[idx] = mode_state(best);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(TPB) void k_user_count(UserArgs ua) {
    const ModeArgs &a = ua.m;
    for (uint64_t s = (uint64_t)blockIdx.x * TPB + threadIdx.x; s < a.n; s += (uint64_t)gridDim.x * TPB) {
        const UserLat l = user_lat(ua, s);
        uint64_t records = 0;
        if (l.valid) walk_chain(l, [&](uint32_t t) { records += node_records(l, a.opts.mode, t); });
        a.sent_len[s] = records;
        a.costs[s] = l.valid ? mode_state_dp(l.sl.state[l.N - 1]) : NBEST_INF;
    }
}

__global__ __launch_bounds__(TPB) void k_user_scan(UserArgs ua) { wg_excl_scan64<TPB>(ua.m.sent_len, ua.m.n); }

__global__ __launch_bounds__(TPB) void k_user_write(UserArgs ua) {
    const ModeArgs &a = ua.m;
    if (a.sent_len[a.n] > a.token_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (TPB / 64);
    for (uint64_t s = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); s < a.n; s += waves) {
        const UserLat l = user_lat(ua, s);
        if (!l.valid) continue;
        uint64_t at = a.sent_len[s + 1];   // the chain is met from its end; every lane walks it, the stores are dealt among the lanes
        const uint64_t lo = a.sent_len[s];
        walk_chain(l, [&](uint32_t t) {
            const uint32_t cnt = node_records(l, a.opts.mode, t);
            if (at - lo < cnt) { at = lo; return; }   // (cannot be: k_user_count walked the same chain)
            at -= cnt;
            if (t >= l.N) {
                const uint4 nd = l.sl.unode[t - l.N];
                const uint32_t bs = l.cbyte[nd.z];
                if (lane == 0) a.tokens[at] = user_record(l.sl.uent[t - l.N], bs, nd.z, nd.w, l.cbyte[nd.w] - bs);
                return;
            }
            if (cnt == 1) {
                if (lane == 0) a.tokens[at] = lat_record(l, t);
                return;
            }
            const int32_t sid = (int32_t)l.nodeA[t].w;
            const uint2 se = l.nodeB[t];
            for (uint32_t c = se.x + lane; c < se.y; c += 64) a.tokens[at + (c - se.x)] = mode_char_record(-sid, c, l.cbyte[c], l.cbyte[c + 1]);
        });
    }
}

int launch_user_measure(const UserArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const unsigned groups = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(a.m.n, 4096));
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.m.n + TPB - 1) / TPB, 1024));
    hipLaunchKernelGGL(k_user_forward, dim3(groups), dim3(FWD_TPB), 0, st, a);
    hipLaunchKernelGGL(k_user_count, dim3(blocks), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_user_scan, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_user_write(const UserArgs &a, void *stream) {
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.m.n + TPB / 64 - 1) / (TPB / 64), 1024));
    hipLaunchKernelGGL(k_user_write, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
