// kanpyo_amd/csrc/kgpu_mode_host.cpp -- kgpu_mode_host: the search / extended mode decode of one lattice (include/kanpyo_gpu.h, "search mode") on the
// host, the definition of what kgpu_mode.hip writes.  HIP-free, compiles alone (with a set_error of the caller's): the penalty, the candidate, the state
// and the records of kgpu_mode_core.h decide every value here as they do on the device; this file adds the loops and the argument checks.
#include <vector>

#include "kgpu_internal.h"
#include "kgpu_mode_core.h"

extern "C" int kgpu_mode_host(const kgpu_lattice *lattice, const uint8_t *utf8, uint64_t len, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols,
                              const kgpu_mode_opts *opts, kgpu_token *tokens, uint64_t token_capacity, uint64_t *n_tokens, int32_t *cost) {
    const char *who = "kgpu_mode_host";
    using namespace kgpu;
    if (n_tokens) *n_tokens = 0;
    if (!lattice || !conn || !opts || !n_tokens || !cost || (len && !utf8) || (token_capacity && !tokens)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (!mode_opts_valid(*opts)) { set_error("%s: mode %u is not 0, 1 or 2, or a reserved word is set", who, opts->mode); return KGPU_ERR_INVALID_ARG; }
    const uint64_t N = lattice->n_nodes, NP = lattice->n_positions;
    if (N < 2 || N >= MODE_MAX_NODES || !lattice->nodes || !lattice->edge_offsets || !lattice->edge_nodes) {
        set_error("%s: a lattice has BOS, EOS and fewer than 2^32 - 1 nodes", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (len >= (1ull << 31)) { set_error("%s: sentence too long", who); return KGPU_ERR_INVALID_ARG; }
    // the characters: each one's byte offset ([C] = len) and the kanji in front of it ([C] = all of them)
    std::vector<uint32_t> cbyte, kanji;
    uint32_t seen = 0;
    for (uint64_t b = 0; b < len;) {
        const uint32_t l = mode_char_bytes(utf8[b]);
        bool ok = (utf8[b] < 0x80u || (utf8[b] >= 0xC2u && utf8[b] <= 0xF4u)) && b + l <= len;
        for (uint32_t k = 1; ok && k < l; ++k) ok = (utf8[b + k] & 0xC0u) == 0x80u;
        if (!ok) { set_error("%s: the text is not UTF-8 at byte %llu", who, (unsigned long long)b); return KGPU_ERR_INVALID_ARG; }
        cbyte.push_back((uint32_t)b); kanji.push_back(seen);
        seen += mode_is_kanji(mode_code_point(utf8 + b)) ? 1u : 0u;
        b += l;
    }
    const uint64_t C = cbyte.size();
    cbyte.push_back((uint32_t)len); kanji.push_back(seen);
    const auto bad = [&](uint64_t t, const char *what) { set_error("%s: node %llu: %s", who, (unsigned long long)t, what); return KGPU_ERR_INVALID_ARG; };
    for (uint64_t p = 0; p < NP; ++p)
        if (lattice->edge_offsets[p + 1] < lattice->edge_offsets[p] || lattice->edge_offsets[p + 1] > N) { set_error("%s: edge offsets run backwards or past the nodes at position %llu", who, (unsigned long long)p); return KGPU_ERR_INVALID_ARG; }
    for (uint64_t t = 0; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        if (nd.end_char < nd.char_pos) return bad(t, "end_char < char_pos");
        if (nd.char_pos >= NP) return bad(t, "starts behind the last position");
        if (nd.end_char > C) return bad(t, "ends behind the text's characters");
        if ((uint64_t)nd.byte_pos + nd.byte_len > len) return bad(t, "bytes beyond the text");
        if ((uint64_t)(uint16_t)nd.left_id >= conn_cols || (uint64_t)(uint16_t)nd.right_id >= conn_rows) return bad(t, "a context id outside the matrix");
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; t && e < lattice->edge_offsets[nd.char_pos + 1]; ++e)
            if (lattice->edge_nodes[e] >= t) return bad(t, "a predecessor that is not in front of it");
    }
    // the forward, node after node: every predecessor is in front of its target
    std::vector<uint64_t> state((size_t)N);
    state[0] = mode_bos_state();
    for (uint64_t t = 1; t < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        const int16_t *col = conn + (size_t)conn_rows * (uint16_t)nd.left_id;
        const uint32_t L = nd.end_char - nd.char_pos;
        const int32_t word = (int32_t)nd.cost + mode_penalty(*opts, nd.cls == KGPU_CLASS_DUMMY, L, kanji[nd.end_char] - kanji[nd.char_pos]);
        uint64_t best = MODE_NONE;
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; e < lattice->edge_offsets[nd.char_pos + 1]; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            const uint64_t key = mode_candidate(mode_state_dp(state[j]), j, word, (int32_t)col[(uint16_t)lattice->nodes[j].right_id]);
            if (key < best) best = key;
        }
        state[(size_t)t] = mode_state(best);
    }
    *cost = mode_state_dp(state[(size_t)(N - 1)]);
    // the chain from EOS along pre: its head is dropped (a chain's nodes descend: it ends)
    uint64_t T = 0;
    for (uint64_t node = N - 1; mode_state_pre(state[(size_t)node]) != MODE_NO_PRE; node = mode_state_pre(state[(size_t)node])) {
        const kgpu_lattice_node &nd = lattice->nodes[node];
        T += mode_record_count(opts->mode, nd.cls, nd.char_pos, nd.end_char);
    }
    *n_tokens = T;
    if (T > token_capacity) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)T, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    uint64_t at = T;
    for (uint64_t node = N - 1; mode_state_pre(state[(size_t)node]) != MODE_NO_PRE; node = mode_state_pre(state[(size_t)node])) {
        const kgpu_lattice_node &nd = lattice->nodes[node];
        const uint32_t cnt = mode_record_count(opts->mode, nd.cls, nd.char_pos, nd.end_char);
        at -= cnt;
        if (cnt == 1) { tokens[at] = nbest_record(nd.cls, nd.id, nd.byte_pos, nd.char_pos, nd.end_char, nd.byte_len); continue; }
        for (uint32_t c = nd.char_pos; c < nd.end_char; ++c) tokens[at + (c - nd.char_pos)] = mode_char_record(nd.id, c, cbyte[c], cbyte[c + 1]);
    }
    return KGPU_OK;
}
