// kanpyo_amd/csrc/kgpu_nbest_host.cpp -- kgpu_nbest_host: the N-best paths of one lattice (include/kanpyo_gpu.h, "N-best paths") on the host, the
// definition of what kgpu_nbest.hip writes.  HIP-free, compiles alone (with a set_error of the caller's): the key, the candidate and the record of
// kgpu_nbest_core.h decide every entry here as they do on the device; this file adds the loops and the argument checks.
#include <algorithm>
#include <vector>

#include "kgpu_internal.h"
#include "kgpu_nbest_core.h"

extern "C" int kgpu_nbest_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, uint32_t n_best,
                               kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs, uint64_t path_capacity,
                               uint64_t *n_paths, uint64_t *n_tokens) {
    const char *who = "kgpu_nbest_host";
    using namespace kgpu;
    if (n_paths) *n_paths = 0;
    if (n_tokens) *n_tokens = 0;
    if (!lattice || !conn || !n_paths || !n_tokens || !tok_offsets || (token_capacity && !tokens) || (path_capacity && !costs)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (n_best < 1 || n_best > KGPU_NBEST_MAX) { set_error("%s: n_best %u is outside 1 .. %d", who, n_best, KGPU_NBEST_MAX); return KGPU_ERR_INVALID_ARG; }
    const uint64_t N = lattice->n_nodes, NP = lattice->n_positions, k = n_best;
    if (N < 2 || N >= NBEST_MAX_NODES || !lattice->nodes || !lattice->edge_offsets || !lattice->edge_nodes) {
        set_error("%s: a lattice has BOS, EOS and fewer than 2^26 nodes", who);
        return KGPU_ERR_INVALID_ARG;
    }
    const auto bad = [&](uint64_t t, const char *what) { set_error("%s: node %llu: %s", who, (unsigned long long)t, what); return KGPU_ERR_INVALID_ARG; };
    for (uint64_t p = 0; p < NP; ++p)
        if (lattice->edge_offsets[p + 1] < lattice->edge_offsets[p] || lattice->edge_offsets[p + 1] > N) { set_error("%s: edge offsets run backwards or past the nodes at position %llu", who, (unsigned long long)p); return KGPU_ERR_INVALID_ARG; }
    for (uint64_t t = 0; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        if (nd.end_char < nd.char_pos) return bad(t, "end_char < char_pos");
        if (nd.char_pos >= NP) return bad(t, "starts behind the last position");
        if ((uint64_t)(uint16_t)nd.left_id >= conn_cols || (uint64_t)(uint16_t)nd.right_id >= conn_rows) return bad(t, "a context id outside the matrix");
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; t && e < lattice->edge_offsets[nd.char_pos + 1]; ++e)
            if (lattice->edge_nodes[e] >= t) return bad(t, "a predecessor that is not in front of it");
    }
    // the lists, node after node: every predecessor is in front of its target
    std::vector<uint64_t> L((size_t)(N * k), NBEST_NONE), cand;
    L[0] = nbest_bos_key();
    for (uint64_t t = 1; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        const int16_t *col = conn + (size_t)conn_rows * (uint16_t)nd.left_id;
        cand.clear();
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; e < lattice->edge_offsets[nd.char_pos + 1]; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            const int32_t cc = col[(uint16_t)lattice->nodes[j].right_id];
            for (uint32_t r = 0; r < k; ++r) {
                const uint64_t key = nbest_candidate(L[(size_t)(j * k + r)], j, r, nd.cost, cc);
                if (key != NBEST_NONE) cand.push_back(key);
            }
        }
        const size_t keep = std::min<size_t>(cand.size(), (size_t)k);
        std::partial_sort(cand.begin(), cand.begin() + keep, cand.end());
        std::copy(cand.begin(), cand.begin() + keep, L.begin() + (size_t)(t * k));
    }
    // the paths: L(EOS), each read back to BOS
    const uint64_t *eos = &L[(size_t)((N - 1) * k)];
    uint64_t P = 0, T = 0;
    std::vector<uint64_t> len;
    for (; P < k && eos[P] != NBEST_NONE; ++P) {
        uint64_t n = 0;
        for (uint64_t node = N - 1, rank = P; node; ++n) { const uint64_t key = L[(size_t)(node * k + rank)]; node = nbest_key_pred(key); rank = nbest_key_rank(key); }
        len.push_back(n);
        T += n;
    }
    *n_paths = P; *n_tokens = T;
    if (P > path_capacity || T > token_capacity) {
        set_error("buffers too small: need %llu paths (capacity %llu) and %llu tokens (capacity %llu)", (unsigned long long)P, (unsigned long long)path_capacity,
                  (unsigned long long)T, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    tok_offsets[0] = 0;
    for (uint64_t p = 0; p < P; ++p) {
        costs[p] = nbest_key_cost(eos[p]);
        tok_offsets[p + 1] = tok_offsets[p] + len[(size_t)p];
        uint64_t at = tok_offsets[p + 1];
        for (uint64_t node = N - 1, rank = p; node;) {
            const kgpu_lattice_node &nd = lattice->nodes[node];
            tokens[--at] = nbest_record(nd.cls, nd.id, nd.byte_pos, nd.char_pos, nd.end_char, nd.byte_len);
            const uint64_t key = L[(size_t)(node * k + rank)];
            node = nbest_key_pred(key); rank = nbest_key_rank(key);
        }
    }
    return KGPU_OK;
}
