// kanpyo_amd/csrc/kgpu_prob.hip -- the lattice probabilities of a batch on the device (include/kanpyo_gpu.h, "lattice probabilities"; not an output of the
// reference: what `mecab -m` and `mecab -l --theta` give), over kept lattices ("The kept-lattice protocol"; kgpu_lattice_dev.h is the view of one).
// kgpu_prob_host.cpp states the rule on the host; both run the statements of kgpu_prob_core.h, whose sums are integer sums and whose maxima are
// maxima: nothing below depends on the order a bucket's slots were filled in, or on which lane met which term.
//
// The launches, on the context's stream:
//   k_prob_forward   one workgroup of FWD_WAVES wavefronts per sentence, k_nbest_forward's frame: position after position, the nodes that start at one position
//                    dealt among the wavefronts, ONE WAVEFRONT PER TARGET, lanes over the predecessors of the position's bucket, 64 per round.  A lane loads its
//                    bucket entry, alpha[j] and its connection cost from the target's matrix column; a wave maximum of doubles, fix(kexp(a - m)), a wave sum of
//                    u64 -- cross-lane operations, no LDS.  A target of at most 64 predecessors keeps a_j in its register between the two passes.
//                    alpha is f64[N] at the head of a slab the kernel takes itself (lat_take_slab); the
//                    slab also holds what the later launches of the call need: beta f64[N] and the best-path bytes u8[N] (marginals), or the sampled nodes
//                    u32[n_samples][C + 2] (samples).
//   k_prob_backward  the mirror: positions descending, one wavefront per node OF THE BUCKET of q, lanes over the nodes that start at q.  A lane's matrix
//                    element lies in its own column (a strided gather, where the forward kernel reads one column).  One thread marks tokenize's path.
//   k_prob_count / k_prob_scan / k_prob_write        the marginals out: a wavefront per sentence filters its nodes in node order
//   k_prob_sample / k_prob_scan_paths / k_prob_write_paths   one wavefront per (sentence, sample) walks back from EOS, the wave arg-max of alpha + w + G on
//                    (value, node); the chosen nodes go to the slab, so the write pass copies and does not draw again
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_lattice_dev.h"
#include "kgpu_prob_core.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t TPB = 256;
constexpr uint32_t FWD_WAVES = 4;   // wavefronts of a forward / backward workgroup

// The slab of a sentence behind its alpha (the bytes: ProbArgs says who needs what)
__host__ __device__ inline uint64_t prob_slab_bytes(uint64_t N, uint64_t C, uint32_t n_samples) {
    return n_samples ? 8 * N + 4 * (C + 2) * n_samples : 16 * N + ((N + 7) & ~7ull);
}

// A sentence's kept lattice with what lies at LAT_OWN: the probability slab (prob_slab_bytes), as the passes behind the forward kernel read it.
struct ProbLat : KeptLat { double *alpha, *beta; uint8_t *best; uint32_t *picks; };
__device__ __forceinline__ ProbLat prob_lat(const ProbArgs &a, uint64_t s) {
    ProbLat l{kept_lat(a.arena, a.desc, s), nullptr, nullptr, nullptr, nullptr};
    if (!l.valid) return l;
    uint8_t *sp = a.arena + l.own;
    l.alpha = (double *)sp;
    l.beta = (double *)(sp + 8ull * l.N); l.best = sp + 16ull * l.N;   // (marginals)
    l.picks = (uint32_t *)(sp + 8ull * l.N);                           // (samples)
    return l;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double wave_max_f64(double v) {   // every lane gets the maximum; exec must be full; no NaN comes here
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = prob_from_bits(shfl_xor64(prob_bits(v), d));
        v = o > v ? o : v;
    }
    return v;
}

// log-sum over the terms term(i), i in [0, cnt), which the lanes take 64 per round: the maximum, then the fixed-point sum around it.  Wave-uniform
// cnt; exec full.  term(i) gives -inf for a term that does not count.  Every lane gets the result (-inf: no term counts).
template <class F>
__device__ __forceinline__ double wave_logsum(uint32_t cnt, uint32_t lane, F &&term) {
    const double ninf = prob_neg_inf();
    if (cnt <= 64) {   // one round: the term stays in its register between the two passes
        const double v = lane < cnt ? term(lane) : ninf;
        const double m = wave_max_f64(v);
        if (!prob_finite(m)) return ninf;
        return prob_logsum(m, wave_sum64(prob_finite(v) ? prob_fix(kexp(v - m)) : 0ull));
    }
    double m = ninf;
    for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
        const double v = i0 + lane < cnt ? term(i0 + lane) : ninf;
        m = v > m ? v : m;
    }
    m = wave_max_f64(m);
    if (!prob_finite(m)) return ninf;
    uint64_t S = 0;
    for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
        const double v = i0 + lane < cnt ? term(i0 + lane) : ninf;
        S += prob_finite(v) ? prob_fix(kexp(v - m)) : 0ull;
    }
    return prob_logsum(m, wave_sum64(S));
}

__device__ __forceinline__ bool listed(const ProbArgs &a, const ProbLat &l, uint32_t t, double log_z, double &p) {
    const double al = l.alpha[t], be = l.beta[t];
    p = prob_marginal(al, be, log_z);
    if (a.select == KGPU_MARGINAL_BEST) return l.best[t] != 0;
    return prob_finite(al) && prob_finite(be) && p >= a.min_prob;
}

}  // namespace

__global__ __launch_bounds__(64 * FWD_WAVES) void k_prob_forward(ProbArgs a) {
    __shared__ unsigned long long slab_off;   // lat_take_slab's word
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6);
    const double theta = a.theta;
    const BatchArgs arena = lat_arena_args(a.ctl, a.arena, a.arena_bytes);
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const KeptLat l = kept_lat<true>(a.arena, a.desc, s);
        if (!l.valid) continue;   // invalid UTF-8, or the lattice itself did not fit: the status says which
        const uint32_t C = l.C;
        const uint64_t off = lat_take_slab(a.desc + LAT_DESC_WORDS * s, prob_slab_bytes(l.N, C, a.n_samples), l.N, PROB_MAX_NODES, &slab_off, arena, a.status + s);
        if (off == LAT_NO_SLAB) continue;
        double *alpha = (double *)(a.arena + off);
        const uint32_t *nb = l.nb, *boff = l.boff;
        const uint4 *nodeA = l.nodeA, *bucket = l.bucket;
        if (threadIdx.x == 0) alpha[0] = 0.0;   // BOS
        __syncthreads();
        for (uint32_t q = 0; q <= C; ++q) {   // the nodes that start at q: independent of each other, their predecessors' alpha is final
            const uint32_t t0 = bcast32(nb[q]), t1 = bcast32(nb[q + 1]), p0 = bcast32(boff[q]), P = bcast32(boff[q + 1]) - p0;
            for (uint32_t t = t0 + wave; t < t1; t += FWD_WAVES) {
                const uint4 nd = nodeA[t];
                const int16_t *col = a.conn + (size_t)a.conn_rows * (nd.x & 0xFFFFu);
                const double v = wave_logsum(P, lane, [&](uint32_t i) {
                    const uint4 e = bucket[p0 + i];
                    const double aj = alpha[e.z];
                    return prob_finite(aj) ? prob_term(aj, theta, (int32_t)col[e.y], (int32_t)nd.y) : prob_neg_inf();
                });
                if (lane == 0) alpha[t] = v;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64 * FWD_WAVES) void k_prob_backward(ProbArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = bcast32(threadIdx.x >> 6);
    const double theta = a.theta;
    for (uint64_t s = blockIdx.x; s < a.n; s += gridDim.x) {
        const ProbLat l = prob_lat(a, s);
        if (!bcast32(l.valid)) continue;
        const uint32_t N = bcast32(l.N), C = bcast32(l.C);
        for (uint32_t t = threadIdx.x; t < N; t += 64 * FWD_WAVES) { l.beta[t] = t == N - 1 ? 0.0 : prob_neg_inf(); l.best[t] = 0; }
        __syncthreads();
        if (threadIdx.x == 0) {   // tokenize's path: its walk over pre, from EOS until a node without one (nobody reads the bytes in this launch)
            uint32_t pos = N - 1, pr, steps = 0;
            while ((pr = l.pre[pos]) != NONE && pr < pos && steps < N) { l.best[pos] = 1; pos = pr; ++steps; }
        }
        for (uint32_t q = C + 1; q-- > 0;) {   // the nodes that end at q: independent of each other, their successors' beta is final
            const uint32_t t0 = bcast32(l.nb[q]), T = bcast32(l.nb[q + 1]) - t0, p0 = bcast32(l.boff[q]), p1 = bcast32(l.boff[q + 1]);
            for (uint32_t p = p0 + wave; p < p1; p += FWD_WAVES) {
                const uint4 e = l.bucket[p];
                const int16_t *row = a.conn + e.y;
                const double v = wave_logsum(T, lane, [&](uint32_t i) {
                    const uint4 nd = l.nodeA[t0 + i];
                    const double bt = l.beta[t0 + i];
                    return prob_finite(bt) ? prob_term(bt, theta, (int32_t)row[(size_t)a.conn_rows * (nd.x & 0xFFFFu)], (int32_t)nd.y) : prob_neg_inf();
                });
                if (lane == 0) l.beta[e.z] = v;
            }
            __syncthreads();
        }
    }
}

// per sentence its records, log_z and best_logprob: a wavefront per sentence
__global__ __launch_bounds__(TPB) void k_prob_count(ProbArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (TPB / 64);
    for (uint64_t s = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); s < a.n; s += waves) {
        const ProbLat l = prob_lat(a, s);
        const double log_z = l.valid ? l.alpha[l.N - 1] : prob_neg_inf();
        const bool reach = prob_finite(log_z);
        uint64_t cnt = 0;
        if (reach)
            for (uint32_t t = 1 + lane; t < l.N; t += 64) { double p; cnt += listed(a, l, t, log_z, p); }
        cnt = wave_sum64(cnt);
        if (lane == 0) {
            a.sent_len[s] = cnt;
            a.log_z[s] = log_z;
            a.best_logprob[s] = reach ? -a.theta * (double)l.eos_dp - log_z : prob_neg_inf();
        }
    }
}

__global__ __launch_bounds__(TPB) void k_prob_scan(ProbArgs a) { wg_excl_scan64<TPB>(a.sent_len, a.n); }

__global__ __launch_bounds__(TPB) void k_prob_write(ProbArgs a) {
    if (a.sent_len[a.n] > a.token_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (TPB / 64);
    for (uint64_t s = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); s < a.n; s += waves) {
        if (a.sent_len[s + 1] == a.sent_len[s]) continue;
        const ProbLat l = prob_lat(a, s);
        const double log_z = l.alpha[l.N - 1];
        uint64_t at = a.sent_len[s];
        for (uint32_t t0 = 1; t0 < l.N; t0 += 64) {   // in node order: a round's records behind those of the rounds before, a lane's behind the lower lanes'
            const uint32_t t = t0 + lane;
            double p = 0.0;
            const bool keep = t < l.N && listed(a, l, t, log_z, p);
            const uint64_t mask = __ballot(keep);
            if (keep) {
                const uint64_t o = at + __popcll(mask & ((1ull << lane) - 1ull));
                a.tokens[o] = lat_record(l, t);
                a.probs[o] = p;
                a.on_best[o] = l.best[t];
            }
            at += __popcll(mask);
        }
    }
}

// one wavefront per (sentence, sample): the walk back from EOS, its nodes (EOS first) into the sentence's slab, its length and cost
__global__ __launch_bounds__(TPB) void k_prob_sample(ProbArgs a) {
    const uint32_t lane = threadIdx.x & 63u, ns = a.n_samples;
    const uint64_t items = a.n * ns, waves = (uint64_t)gridDim.x * (TPB / 64);
    const double theta = a.theta;
    for (uint64_t i = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); i < items; i += waves) {
        const uint64_t s = i / ns;
        const uint32_t r = (uint32_t)(i - s * ns);
        const ProbLat l = prob_lat(a, s);
        const bool reach = bcast32(l.valid && prob_finite(l.alpha[l.N - 1]));
        if (r == 0 && lane == 0) a.path_offsets[s] = reach ? ns : 0;
        if (!reach) { if (lane == 0) { a.path_len[i] = 0; a.path_cost[i] = 0; } continue; }
        const uint32_t N = bcast32(l.N), cap = bcast32(l.C) + 2;
        uint32_t *picks = l.picks + (uint64_t)r * cap;
        uint32_t t = N - 1, len = 0;
        int64_t cost = 0;
        while (t != 0 && len < cap) {   // (a path has at most C + 1 nodes behind BOS: the bound is the slab's)
            const uint4 nd = l.nodeA[t];
            const uint32_t q = l.nodeB[t].x;
            const int16_t *col = a.conn + (size_t)a.conn_rows * (nd.x & 0xFFFFu);
            const uint32_t p0 = bcast32(l.boff[q]), P = bcast32(l.boff[q + 1]) - p0;
            const uint64_t ht = prob_hash_target(a.seed, a.sent_base + s, r, t);
            double bv = prob_neg_inf();
            uint32_t bj = NONE;
            for (uint32_t i0 = 0; i0 < P; i0 += 64) {
                if (i0 + lane >= P) continue;
                const uint4 e = l.bucket[p0 + i0 + lane];
                const double aj = l.alpha[e.z];
                if (!prob_finite(aj)) continue;
                const double v = prob_term(aj, theta, (int32_t)col[e.y], (int32_t)nd.y) + prob_gumbel(ht, e.z);
                if (v > bv || (v == bv && e.z < bj)) { bv = v; bj = e.z; }
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {   // the wave arg-max on (value, node): the lower node at a tie
                const double ov = prob_from_bits(shfl_xor64(prob_bits(bv), d));
                const uint32_t oj = (uint32_t)__shfl_xor((int)bj, d, 64);
                if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
            }
            bj = bcast32(bj);
            if (bj == NONE || bj >= t) break;   // cannot be on a lattice the general kernel built: alpha[t] says a predecessor has a forward value, and it is in front of
                                                // t.  The host rule refuses such a lattice (KGPU_ERR_INVALID_ARG) before it walks; here the walk only has to end: the
                                                // two do NOT define the same result for it, and the byte-for-byte claim covers consistent lattices alone
            if (lane == 0) picks[len] = t;
            cost += (int32_t)col[l.nodeA[bj].x >> 16] + (int32_t)nd.y;
            ++len;
            t = bj;
        }
        if (lane == 0) { a.path_len[i] = len; a.path_cost[i] = prob_sat32(cost); }
    }
}

__global__ __launch_bounds__(TPB) void k_prob_scan_paths(ProbArgs a) {
    wg_excl_scan64<TPB>(a.path_len, a.n * a.n_samples);
    wg_excl_scan64<TPB>(a.path_offsets, a.n);
}

__global__ __launch_bounds__(TPB) void k_prob_write_paths(ProbArgs a) {
    const uint32_t lane = threadIdx.x & 63u, ns = a.n_samples;
    const uint64_t items = a.n * ns, waves = (uint64_t)gridDim.x * (TPB / 64);
    if (a.path_len[items] > a.token_cap || a.path_offsets[a.n] > a.path_cap) return;   // the host reports KGPU_ERR_CAPACITY with the sizes needed
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tok_offsets[a.path_offsets[a.n]] = a.path_len[items];
    for (uint64_t i = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); i < items; i += waves) {
        const uint64_t s = i / ns;
        const uint32_t r = (uint32_t)(i - s * ns);
        if (r >= a.path_offsets[s + 1] - a.path_offsets[s]) continue;
        const ProbLat l = prob_lat(a, s);
        const uint64_t p = a.path_offsets[s] + r, at = a.path_len[i], len = a.path_len[i + 1] - at;
        if (lane == 0) { a.tok_offsets[p] = at; a.costs[p] = a.path_cost[i]; }
        const uint32_t *picks = l.picks + (uint64_t)r * (l.C + 2);
        for (uint64_t k = lane; k < len; k += 64) {   // the walk met the path from its end
            a.tokens[at + k] = lat_record(l, picks[len - 1 - k]);
        }
    }
}

namespace {
unsigned groups_of(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n, 4096)); }
unsigned wave_blocks(uint64_t items) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + TPB / 64 - 1) / (TPB / 64), 4096)); }
}  // namespace

int launch_prob_marginals_measure(const ProbArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_prob_forward, dim3(groups_of(a.n)), dim3(64 * FWD_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_prob_backward, dim3(groups_of(a.n)), dim3(64 * FWD_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_prob_count, dim3(wave_blocks(a.n)), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_prob_scan, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_prob_marginals_write(const ProbArgs &a, void *stream) {
    hipLaunchKernelGGL(k_prob_write, dim3(wave_blocks(a.n)), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
int launch_prob_samples_measure(const ProbArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_prob_forward, dim3(groups_of(a.n)), dim3(64 * FWD_WAVES), 0, st, a);
    hipLaunchKernelGGL(k_prob_sample, dim3(wave_blocks(a.n * a.n_samples)), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_prob_scan_paths, dim3(1), dim3(TPB), 0, st, a);
    return (int)hipGetLastError();
}
int launch_prob_samples_write(const ProbArgs &a, void *stream) {
    hipLaunchKernelGGL(k_prob_write_paths, dim3(wave_blocks(a.n * a.n_samples)), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// (tests) kexp (which = 0) or klog (which = 1) over an array, on the device
__global__ __launch_bounds__(TPB) void k_prob_eval(const double *x, uint64_t n, double *out, uint32_t which) {
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) out[i] = which ? klog(x[i]) : kexp(x[i]);
}
int launch_prob_eval(const double *d_x, uint64_t n, double *d_out, uint32_t which, void *stream) {
    hipLaunchKernelGGL(k_prob_eval, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + TPB - 1) / TPB, 1024))), dim3(TPB), 0, (hipStream_t)stream, d_x, n, d_out, which);
    return (int)hipGetLastError();
}

}  // namespace kgpu
