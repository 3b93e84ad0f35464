// kanpyo_amd/csrc/kgpu_graphviz.hip -- the `kanpyo graphviz` output of a batch on the device (reference src/graphviz.rs:30-163 behind
// src/bin/kanpyo.rs:127-148): one DOT document per sentence, byte for byte what Graphviz::graphviz(dpi, full_state) prints, over kept lattices
// ("The kept-lattice protocol"; kgpu_lattice_dev.h is the view of one).  kanpyo_amd/lattice.py::graphviz states every case in Python.
//
// Four launches on the context's stream, one workgroup per sentence at a time:
//   k_gv_prepare  bests (the backtrace over `pre`, graphviz.rs:31-35), the nodes sorted by (end position, index) -- Lattice.edges as one array.  The
//                 sort is needed: the emit phase hands out a bucket's slots by atomicAdd across lanes that hold different start positions, so slot order
//                 is NOT the reference's insertion order (kgpu_lattice_dump sorts its buckets on the host for the same reason) -- and the visible nodes with their ids: every node in insertion order (full_state), or
//                 what the reference's BFS from the last node reaches (graphviz.rs:10-28: one backward pass over end positions; unknown words only
//                 on the best path) ranked by the BTreeSet's order -- (class, id, byte position) decides it for distinct nodes: a 64-bit key, sorted
//   k_gv_len      every node line's and every target's edge lines' bytes, scanned inside the sentence; the document's bytes -> sent_len[s]
//   k_gv_scan     one workgroup: exclusive scan of sent_len in place; [n] = the batch's bytes
//   k_gv_write    the same generators as k_gv_len, storing: nothing when the batch's bytes exceed the capacity
// All offsets are 64-bit, inside a sentence too.  Exactness before speed: a thread renders a whole node line, or all edge lines of one target.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_lattice_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t F_BEST = 1u, F_VISIBLE = 2u;

// A sentence's kept lattice with what lies at LAT_OWN -- its visible nodes, V -- its text, and the passes' arrays in the scratch behind slab N
// (kgpu_internal.h: lat_scratch_bytes) and in slab A's backtrace array.
struct GvLat : KeptLat {
    uint32_t V;
    const uint8_t *text;
    uint32_t *reach;                 // KeptLat::path: u32 per position
    uint64_t *sorted, *key, *noff, *eoff;
    uint32_t *vis, *order, *flags;
};
__device__ __forceinline__ GvLat gv_lat(const GraphvizArgs &a, uint64_t s) {
    GvLat l{kept_lat(a.arena, a.desc, s), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!l.valid) return l;
    l.V = (uint32_t)l.own;
    l.text = a.utf8 + a.offsets[s];
    l.reach = l.path;
    const uint64_t N = l.N;
    l.sorted = (uint64_t *)l.scratch; l.key = l.sorted + (N + 1); l.noff = l.key + (N + 1); l.eoff = l.noff + (N + 1);
    l.vis = (uint32_t *)(l.eoff + (N + 1)); l.order = l.vis + N; l.flags = l.order + N;
    return l;
}
__device__ __forceinline__ int32_t node_sid(const GvLat &l, uint32_t t) { return (int32_t)l.nodeA[t].w; }   // > 0 known, < 0 unknown, 0 BOS / EOS

// Ascending sort of arr[0 .. n) by the whole workgroup: the bitonic network whose comparators all put the smaller element at the lower index (a merge
// starts with the mirrored step), so elements past n are +infinity that never move: a comparator that reaches past n is skipped.
__device__ void wg_sort64(uint64_t *arr, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    auto cmpswap = [&](uint64_t i, uint64_t j) {
        const uint64_t x = arr[i], y = arr[j];
        if (y < x) { arr[i] = y; arr[j] = x; }
    };
    uint64_t p2 = 1;
    while (p2 < n) p2 <<= 1;
    __syncthreads();
    for (uint64_t k = 2; k <= p2; k <<= 1) {
        const uint64_t h = k >> 1;
        for (uint64_t x = tid; x < p2 / 2; x += TPB) {
            const uint64_t b = x / h, o = x % h, i = b * k + o, j = b * k + (k - 1 - o);
            if (j < n) cmpswap(i, j);
        }
        __syncthreads();
        for (uint64_t st = k >> 2; st > 0; st >>= 1) {
            for (uint64_t x = tid; x < p2 / 2; x += TPB) {
                const uint64_t i = (x / st) * 2 * st + x % st, j = i + st;
                if (j < n) cmpswap(i, j);
            }
            __syncthreads();
        }
    }
}

// ---- the text, written once: a sink either counts or stores
struct Count {
    uint64_t n = 0;
    __device__ __forceinline__ void ch(uint32_t) { ++n; }
    __device__ __forceinline__ void lit(const char *, uint32_t len) { n += len; }
    __device__ __forceinline__ void mem(const uint8_t *, uint32_t len) { n += len; }
};
struct Store {
    uint8_t *p;
    __device__ __forceinline__ void ch(uint32_t c) { *p++ = (uint8_t)c; }
    __device__ __forceinline__ void lit(const char *s, uint32_t len) { for (uint32_t i = 0; i < len; ++i) *p++ = (uint8_t)s[i]; }
    __device__ __forceinline__ void mem(const uint8_t *s, uint32_t len) { for (uint32_t i = 0; i < len; ++i) *p++ = s[i]; }
};
#define GV_LIT(sink, s) (sink).lit(s, (uint32_t)sizeof(s) - 1)
template <class S>
__device__ __forceinline__ void put_u64(S &o, uint64_t v) {
    char buf[20];
    uint32_t k = 0;
    do { buf[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) o.ch((uint8_t)buf[--k]);
}
template <class S>
__device__ __forceinline__ void put_i32(S &o, int32_t v) {
    if (v < 0) { o.ch('-'); put_u64(o, (uint64_t)(-(int64_t)v)); } else put_u64(o, (uint64_t)v);
}

template <class S>
__device__ void put_header(S &o, uint64_t dpi) {   // graphviz.rs:36-40
    GV_LIT(o, "graph lattice {\ndpi=");
    put_u64(o, dpi);
    GV_LIT(o, ";\ngraph [style=filled, splines=true, overlap=false, fontsize=30, rankdir=LR]\n"
              "edge [fontname=Helvetica, fontcolor=red, color=\"#606060\"]\n"
              "node [shape=box, style=filled, fillcolor=\"#e8e8f0\", fontname=Helvetica]\n");
}

// The line of visible node `vid` (graphviz.rs:55-119).
template <class S>
__device__ void put_node(S &o, const GraphvizArgs &a, const GvLat &l, uint32_t vid) {
    const uint32_t t = l.order[vid];
    const int32_t sid = node_sid(l, t);
    put_u64(o, vid);
    GV_LIT(o, " [label=\"");
    if (sid == 0) {
        if (vid == 0) GV_LIT(o, "BOS"); else GV_LIT(o, "EOS");   // by the visible id, whatever the node is (graphviz.rs:90-96)
    } else {
        const uint2 se = l.nodeB[t];
        const uint32_t b0 = l.cbyte[se.x], b1 = l.cbyte[se.y];
        o.mem(l.text + b0, b1 - b0);
        o.ch('\n');
        const uint32_t row = feature_row(sid > 0, a.n_morph, (uint32_t)(sid > 0 ? sid : -sid));
        const uint32_t f0 = a.label_off[row], f1 = a.label_off[row + 1];
        o.mem(a.label + f0, f1 - f0);
        o.ch('\n');
        put_i32(o, (int32_t)l.nodeA[t].y);
    }
    GV_LIT(o, "\", shape=");
    const bool ring = sid == 0 || (l.flags[t] & F_BEST);
    if (ring) GV_LIT(o, "ellipse"); else if (sid > 0) GV_LIT(o, "box"); else GV_LIT(o, "diamond");
    GV_LIT(o, ", color=");
    if (sid == 0) GV_LIT(o, "blue"); else if (sid > 0) GV_LIT(o, "black"); else GV_LIT(o, "red");
    if (ring) GV_LIT(o, ", peripheries=2]\n"); else GV_LIT(o, "]\n");
}

// The edge lines into the k-th node by (end position, index) (graphviz.rs:120-161): from every visible node of edges[its start], ascending.
template <class S>
__device__ void put_edges(S &o, const GraphvizArgs &a, const GvLat &l, uint32_t k) {
    if (l.C == 0) return;   // "": BOS and EOS compare equal, the id map holds one of them and from_id == id skips the pair (graphviz.rs:120-124,138-140)
    const uint32_t t = (uint32_t)l.sorted[k];
    const uint32_t nid = l.vis[t];
    if (nid == NONE) return;
    const uint32_t st = l.nodeB[t].x;
    const bool tb = node_sid(l, t) == 0 || (l.flags[t] & F_BEST);
    const int16_t *col = a.conn + (size_t)a.conn_rows * (l.nodeA[t].x & 0xFFFFu);
    for (uint32_t j = l.boff[st], je = l.boff[st + 1]; j < je; ++j) {
        const uint32_t f = (uint32_t)l.sorted[j];
        const uint32_t fid = l.vis[f];
        if (fid == NONE || fid == nid) continue;
        put_u64(o, fid);
        GV_LIT(o, " -- ");
        put_u64(o, nid);
        GV_LIT(o, " [label=\"");
        put_i32(o, (int32_t)col[l.nodeA[f].x >> 16]);   // ConnectionTable::get(from.right_id, node.left_id), connection.rs:12-14
        const bool fb = node_sid(l, f) == 0 || (l.flags[f] & F_BEST);
        if (tb && fb) GV_LIT(o, "\", style=bold, color=blue, fontcolor=blue]\n"); else GV_LIT(o, "\"]\n");
    }
}

}  // namespace

__global__ __launch_bounds__(TPB) void k_gv_prepare(GraphvizArgs a) {
    __shared__ uint32_t nvis_s;
    const uint32_t tid = threadIdx.x;
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const GvLat l = gv_lat(a, s);
        if (!l.valid) continue;   // (workgroup-uniform)
        const uint32_t N = l.N, C = l.C;
        __syncthreads();
        for (uint32_t t = tid; t < N; t += TPB) {
            l.flags[t] = 0; l.vis[t] = NONE; l.order[t] = NONE;
            const uint32_t end = t == N - 1 ? C + 1 : l.nodeB[t].y;   // EOS: edges[C + 1] (lattice.rs:165-175)
            l.sorted[t] = ((uint64_t)end << 32) | t;
        }
        for (uint32_t p = tid; p <= C; p += TPB) l.reach[p] = p == C;
        if (tid == 0) nvis_s = 0;
        __syncthreads();
        if (tid == 0) {   // bests: the backtrace of Lattice::viterbi (lattice.rs:144-153)
            uint32_t pos = N - 1, pr, steps = 0;
            while ((pr = l.pre[pos]) != NONE && steps++ < N) { l.flags[pos] |= F_BEST; pos = pr; }
        }
        wg_sort64(l.sorted, N);
        uint32_t V;
        if (a.full_state) {
            for (uint32_t t = tid; t < N; t += TPB) { l.vis[t] = t; l.order[t] = t; }
            V = N;
        } else {
            if (C == 0) {   // "": the BFS visits EOS and finds BOS equal to it
                if (tid == 0) l.flags[N - 1] |= F_VISIBLE;
            } else {
                if (tid == 0) l.flags[N - 1] |= F_VISIBLE;
                __syncthreads();
                // a node is visited when it ends where a visited node starts (graphviz.rs:18-25): end positions downwards, a word starts before it ends
                for (uint32_t p = C + 1; p-- > 0;) {
                    if (l.reach[p]) {   // (workgroup-uniform: written before the barrier below)
                        for (uint32_t j = l.boff[p] + tid, je = l.boff[p + 1]; j < je; j += TPB) {
                            const uint32_t t = (uint32_t)l.sorted[j];
                            if (node_sid(l, t) >= 0 || (l.flags[t] & F_BEST)) { l.flags[t] |= F_VISIBLE; l.reach[l.nodeB[t].x] = 1; }
                        }
                    }
                    __syncthreads();
                }
            }
            __syncthreads();
            auto key_of = [&](uint32_t t) {   // the derived Ord of Node (node.rs:6-24): variant, then id, then byte position
                const int32_t sid = node_sid(l, t);
                const uint64_t cls = sid == 0 ? 0 : sid > 0 ? 1 : 2, id = (uint64_t)(sid < 0 ? -(int64_t)sid : sid);
                return (cls << 62) | (id << 31) | (uint64_t)l.cbyte[l.nodeB[t].x];
            };
            uint32_t mine = 0;
            for (uint32_t t = tid; t < N; t += TPB) {
                const bool v = (l.flags[t] & F_VISIBLE) != 0;
                l.key[t] = v ? key_of(t) : ~0ull;
                mine += v;
            }
            if (mine) atomicAdd(&nvis_s, mine);
            wg_sort64(l.key, N);
            V = nvis_s;
            for (uint32_t t = tid; t < N; t += TPB) {
                if (!(l.flags[t] & F_VISIBLE)) continue;
                const uint64_t kk = key_of(t);
                uint32_t lo = 0, hi = V;   // the rank of kk among the V sorted keys
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (l.key[mid] < kk) lo = mid + 1; else hi = mid; }
                l.vis[t] = lo; l.order[lo] = t;
            }
        }
        if (tid == 0) a.desc[LAT_DESC_WORDS * s + LAT_OWN] = V;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TPB) void k_gv_len(GraphvizArgs a) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const GvLat l = gv_lat(a, s);
        if (!l.valid) { if (tid == 0) a.sent_len[s] = 0; continue; }
        for (uint32_t r = tid; r < l.V; r += TPB) { Count c; put_node(c, a, l, r); l.noff[r] = c.n; }
        for (uint32_t k = tid; k < l.N; k += TPB) { Count c; put_edges(c, a, l, k); l.eoff[k] = c.n; }
        const uint64_t nodes = wg_excl_scan64<TPB>(l.noff, l.V), edges = wg_excl_scan64<TPB>(l.eoff, l.N);
        if (tid == 0) { Count h; put_header(h, a.dpi); a.sent_len[s] = h.n + nodes + edges + 2; }
    }
}

// (the pattern of k_lines_scan, kgpu_format.hip)
__global__ __launch_bounds__(TPB) void k_gv_scan(GraphvizArgs a) {
    wg_excl_scan64<TPB>(a.sent_len, a.n);
}

__global__ __launch_bounds__(TPB) void k_gv_write(GraphvizArgs a) {
    if (a.sent_len[a.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint32_t tid = threadIdx.x;
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const GvLat l = gv_lat(a, s);
        if (!l.valid) continue;
        uint8_t *doc = a.text + a.sent_len[s];
        Count h; put_header(h, a.dpi);
        uint8_t *nodes = doc + h.n, *edges = nodes + l.noff[l.V], *foot = edges + l.eoff[l.N];
        if (tid == 0) { Store o{doc}; put_header(o, a.dpi); }
        if (tid == 1) { foot[0] = '}'; foot[1] = '\n'; }
        for (uint32_t r = tid; r < l.V; r += TPB) { Store o{nodes + l.noff[r]}; put_node(o, a, l, r); }
        for (uint32_t k = tid; k < l.N; k += TPB) { Store o{edges + l.eoff[k]}; put_edges(o, a, l, k); }
    }
}

int launch_graphviz_measure(const GraphvizArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(a.n, 4096));
    hipLaunchKernelGGL(k_gv_prepare, dim3(blocks), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_gv_len, dim3(blocks), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_gv_scan, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_graphviz_write(const GraphvizArgs &a, void *stream) {
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(a.n, 4096));
    hipLaunchKernelGGL(k_gv_write, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
