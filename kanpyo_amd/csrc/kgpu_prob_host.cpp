// kanpyo_amd/csrc/kgpu_prob_host.cpp -- kgpu_marginals_host, kgpu_samples_host: the lattice probabilities of one lattice (include/kanpyo_gpu.h, "lattice
// probabilities") on the host, the definition of what kgpu_prob.hip writes.  HIP-free, compiles alone (with a set_error of the caller's): the functions of
// kgpu_prob_core.h decide every number here as they do on the device; this file adds the loops and the argument checks.
#include <vector>

#include "kgpu_internal.h"
#include "kgpu_prob_core.h"

namespace {

using namespace kgpu;

// The checked lattice with its forward values: what both calls start from.
struct Fwd {
    uint64_t N = 0;
    std::vector<uint32_t> s0, s1;   // the nodes that start at position p (BOS left out): [s0[p], s1[p])
    std::vector<double> alpha;
};

int bad_arg(const char *who, const char *what) { set_error("%s: %s", who, what); return KGPU_ERR_INVALID_ARG; }

int forward(const char *who, const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, double theta, Fwd &f) {
    if (!(theta > 0.0) || !(theta <= PROB_THETA_MAX)) return bad_arg(who, "theta is not a double above 0 and at most 2^64");
    const uint64_t N = lattice->n_nodes, NP = lattice->n_positions;
    if (N < 2 || N >= PROB_MAX_NODES || !lattice->nodes || !lattice->edge_offsets || !lattice->edge_nodes) return bad_arg(who, "a lattice has BOS, EOS and fewer than 2^24 nodes");
    const auto bad = [&](uint64_t t, const char *what) { set_error("%s: node %llu: %s", who, (unsigned long long)t, what); return KGPU_ERR_INVALID_ARG; };
    for (uint64_t p = 0; p < NP; ++p)
        if (lattice->edge_offsets[p + 1] < lattice->edge_offsets[p] || lattice->edge_offsets[p + 1] > N) { set_error("%s: edge offsets run backwards or past the nodes at position %llu", who, (unsigned long long)p); return KGPU_ERR_INVALID_ARG; }
    f.N = N;
    f.s0.assign((size_t)NP, 0); f.s1.assign((size_t)NP, 0);
    for (uint64_t t = 0; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        if (nd.end_char < nd.char_pos) return bad(t, "end_char < char_pos");
        if (nd.char_pos >= NP || nd.end_char >= NP) return bad(t, "starts or ends behind the last position");
        if ((uint64_t)(uint16_t)nd.left_id >= conn_cols || (uint64_t)(uint16_t)nd.right_id >= conn_rows) return bad(t, "a context id outside the matrix");
        if (t && nd.char_pos < lattice->nodes[t - 1].char_pos) return bad(t, "starts in front of the node before it");
        if (t && t + 1 < N && nd.end_char == nd.char_pos) return bad(t, "a node without characters that is neither BOS nor EOS");
        if (nd.pre >= 0 && (uint64_t)nd.pre >= t) return bad(t, "a best predecessor that is not in front of it");
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; t && e < lattice->edge_offsets[nd.char_pos + 1]; ++e)
            if (lattice->edge_nodes[e] >= t) return bad(t, "a predecessor that is not in front of it");
        if (t) { if (f.s1[nd.char_pos] == 0) f.s0[nd.char_pos] = (uint32_t)t; f.s1[nd.char_pos] = (uint32_t)t + 1; }
    }
    // alpha, node after node: every predecessor is in front of its target
    f.alpha.assign((size_t)N, prob_neg_inf());
    f.alpha[0] = 0.0;
    for (uint64_t t = 1; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        const int16_t *col = conn + (size_t)conn_rows * (uint16_t)nd.left_id;
        const uint32_t e0 = lattice->edge_offsets[nd.char_pos], e1 = lattice->edge_offsets[nd.char_pos + 1];
        double m = prob_neg_inf();
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            if (!prob_finite(f.alpha[j])) continue;
            const double a = prob_term(f.alpha[j], theta, col[(uint16_t)lattice->nodes[j].right_id], nd.cost);
            if (a > m) m = a;
        }
        if (!prob_finite(m)) continue;
        uint64_t S = 0;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            if (!prob_finite(f.alpha[j])) continue;
            S += prob_fix(kexp(prob_term(f.alpha[j], theta, col[(uint16_t)lattice->nodes[j].right_id], nd.cost) - m));
        }
        f.alpha[(size_t)t] = prob_logsum(m, S);
    }
    return KGPU_OK;
}

}  // namespace

extern "C" int kgpu_marginals_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, double theta, uint32_t select,
                                   double min_prob, kgpu_token *tokens, uint64_t token_capacity, double *probs, uint8_t *on_best, double *log_z,
                                   double *best_logprob, uint64_t *n_tokens) {
    const char *who = "kgpu_marginals_host";
    if (n_tokens) *n_tokens = 0;
    if (!lattice || !conn || !n_tokens || !log_z || !best_logprob || (token_capacity && (!tokens || !probs || !on_best))) return bad_arg(who, "null argument");
    if (select != KGPU_MARGINAL_BEST && select != KGPU_MARGINAL_ALL) return bad_arg(who, "select is neither KGPU_MARGINAL_BEST nor KGPU_MARGINAL_ALL");
    if (!(min_prob >= 0.0 && min_prob <= 1.0)) return bad_arg(who, "min_prob is outside [0, 1]");
    Fwd f;
    int rc;
    if ((rc = forward(who, lattice, conn, conn_rows, conn_cols, theta, f))) return rc;
    const uint64_t N = f.N;
    *log_z = f.alpha[(size_t)N - 1];
    *best_logprob = prob_neg_inf();
    if (!prob_finite(*log_z)) return KGPU_OK;   // EOS is not reachable: no records
    *best_logprob = -theta * (double)lattice->nodes[N - 1].dp - *log_z;
    // beta, by descending end position: a node's successors start where it ends, and end behind that
    std::vector<double> beta((size_t)N, prob_neg_inf());
    beta[(size_t)N - 1] = 0.0;
    for (uint64_t q = lattice->n_positions; q-- > 0;)
        for (uint32_t e = lattice->edge_offsets[q]; e < lattice->edge_offsets[q + 1]; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            if (j == N - 1 || lattice->nodes[j].end_char != q) continue;   // (the dump lists EOS behind the last position)
            const int32_t right = (uint16_t)lattice->nodes[j].right_id;
            double m = prob_neg_inf();
            for (uint32_t t = f.s0[q]; t < f.s1[q]; ++t) {
                if (!prob_finite(beta[t])) continue;
                const kgpu_lattice_node &nd = lattice->nodes[t];
                const double b = prob_term(beta[t], theta, conn[(size_t)conn_rows * (uint16_t)nd.left_id + right], nd.cost);
                if (b > m) m = b;
            }
            if (!prob_finite(m)) continue;
            uint64_t S = 0;
            for (uint32_t t = f.s0[q]; t < f.s1[q]; ++t) {
                if (!prob_finite(beta[t])) continue;
                const kgpu_lattice_node &nd = lattice->nodes[t];
                S += prob_fix(kexp(prob_term(beta[t], theta, conn[(size_t)conn_rows * (uint16_t)nd.left_id + right], nd.cost) - m));
            }
            beta[j] = prob_logsum(m, S);
        }
    // the best path: tokenize's walk over pre, from EOS until a node without one
    std::vector<uint8_t> best((size_t)N, 0);
    {
        uint64_t pos = N - 1, steps = 0;
        for (int32_t pr; (pr = lattice->nodes[pos].pre) >= 0 && steps < N; ++steps) { best[(size_t)pos] = 1; pos = (uint64_t)pr; }
    }
    const auto listed = [&](uint64_t t) {
        if (select == KGPU_MARGINAL_BEST) return best[(size_t)t] != 0;
        return prob_finite(f.alpha[(size_t)t]) && prob_finite(beta[(size_t)t]) && prob_marginal(f.alpha[(size_t)t], beta[(size_t)t], *log_z) >= min_prob;
    };
    uint64_t T = 0;
    for (uint64_t t = 1; t < N; ++t) T += listed(t);
    *n_tokens = T;
    if (T > token_capacity) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)T, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    uint64_t at = 0;
    for (uint64_t t = 1; t < N; ++t) {
        if (!listed(t)) continue;
        const kgpu_lattice_node &nd = lattice->nodes[t];
        tokens[at] = nbest_record(nd.cls, nd.id, nd.byte_pos, nd.char_pos, nd.end_char, nd.byte_len);
        probs[at] = prob_marginal(f.alpha[(size_t)t], beta[(size_t)t], *log_z);
        on_best[at] = best[(size_t)t];
        ++at;
    }
    return KGPU_OK;
}

extern "C" int kgpu_samples_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, double theta, uint32_t n_samples,
                                 uint64_t seed, uint64_t sentence_index, kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs,
                                 uint64_t path_capacity, uint64_t *n_paths, uint64_t *n_tokens) {
    const char *who = "kgpu_samples_host";
    if (n_paths) *n_paths = 0;
    if (n_tokens) *n_tokens = 0;
    if (!lattice || !conn || !n_paths || !n_tokens || !tok_offsets || (token_capacity && !tokens) || (path_capacity && !costs)) return bad_arg(who, "null argument");
    if (n_samples < 1 || n_samples > KGPU_SAMPLES_MAX) { set_error("%s: n_samples %u is outside 1 .. %d", who, n_samples, KGPU_SAMPLES_MAX); return KGPU_ERR_INVALID_ARG; }
    Fwd f;
    int rc;
    if ((rc = forward(who, lattice, conn, conn_rows, conn_cols, theta, f))) return rc;
    const uint64_t N = f.N;
    if (!prob_finite(f.alpha[(size_t)N - 1])) { tok_offsets[0] = 0; return KGPU_OK; }   // EOS is not reachable: no paths
    // the walks, each back from EOS: the predecessor with the largest alpha + w + G, the lower node at a tie
    std::vector<uint32_t> nodes;
    std::vector<uint64_t> ends;
    std::vector<int32_t> cost;
    for (uint32_t i = 0; i < n_samples; ++i) {
        int64_t c = 0;
        for (uint64_t t = N - 1, steps = 0; t && steps < N; ++steps) {
            const kgpu_lattice_node &nd = lattice->nodes[t];
            const int16_t *col = conn + (size_t)conn_rows * (uint16_t)nd.left_id;
            const uint64_t ht = prob_hash_target(seed, sentence_index, i, t);
            double bv = prob_neg_inf();
            uint32_t bj = 0xFFFFFFFFu;
            int32_t bc = 0;
            for (uint32_t e = lattice->edge_offsets[nd.char_pos]; e < lattice->edge_offsets[nd.char_pos + 1]; ++e) {
                const uint32_t j = lattice->edge_nodes[e];
                if (!prob_finite(f.alpha[j])) continue;
                const int32_t cc = col[(uint16_t)lattice->nodes[j].right_id];
                const double v = prob_term(f.alpha[j], theta, cc, nd.cost) + prob_gumbel(ht, j);
                if (v > bv || (v == bv && j < bj)) { bv = v; bj = j; bc = cc + nd.cost; }
            }
            if (bj == 0xFFFFFFFFu) return bad_arg(who, "a node with a forward value and no predecessor that has one");   // (cannot be: alpha says there is one.  The device walk just ends there: kgpu_prob.hip)
            nodes.push_back((uint32_t)t);
            c += bc;
            t = bj;
        }
        ends.push_back(nodes.size());
        cost.push_back(prob_sat32(c));
    }
    const uint64_t P = n_samples, T = nodes.size();
    *n_paths = P; *n_tokens = T;
    if (P > path_capacity || T > token_capacity) {
        set_error("buffers too small: need %llu paths (capacity %llu) and %llu tokens (capacity %llu)", (unsigned long long)P, (unsigned long long)path_capacity,
                  (unsigned long long)T, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    tok_offsets[0] = 0;
    for (uint64_t p = 0; p < P; ++p) {
        costs[p] = cost[(size_t)p];
        tok_offsets[p + 1] = ends[(size_t)p];
        uint64_t at = ends[(size_t)p];   // the walk met the path from its end
        for (uint64_t k = p ? ends[(size_t)p - 1] : 0; k < ends[(size_t)p]; ++k) {
            const kgpu_lattice_node &nd = lattice->nodes[nodes[(size_t)k]];
            tokens[--at] = nbest_record(nd.cls, nd.id, nd.byte_pos, nd.char_pos, nd.end_char, nd.byte_len);
        }
    }
    return KGPU_OK;
}

// (tests) kexp and klog over arrays
extern "C" void kgpu_prob_exp_host(const double *x, uint64_t n, double *out) { for (uint64_t i = 0; i < n; ++i) out[i] = kgpu::kexp(x[i]); }
extern "C" void kgpu_prob_log_host(const double *x, uint64_t n, double *out) { for (uint64_t i = 0; i < n; ++i) out[i] = kgpu::klog(x[i]); }
