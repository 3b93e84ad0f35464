// kanpyo_amd/csrc/kgpu_user_host.cpp -- kgpu_userdict_host: the decode of one lattice widened by a user dictionary's matches (include/kanpyo_gpu.h, "user
// dictionary") on the host, the definition of what kgpu_user.hip writes.  HIP-free, compiles with kgpu_user_table.cpp alone (and a set_error of the
// caller's): the table, the match, the withdrawal and the record of kgpu_user_core.h and the penalty, candidate and state of kgpu_mode_core.h decide every
// value here as they do on the device; this file adds the loops and the argument checks.
#include <vector>

#include "kgpu_internal.h"
#include "kgpu_user_core.h"

extern "C" int kgpu_userdict_host(const kgpu_lattice *lattice, const uint8_t *utf8, uint64_t len, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols,
                                  const uint8_t *invoke, const uint8_t *keys, const uint64_t *key_offsets, const uint16_t *left_id, const uint16_t *right_id,
                                  const int16_t *cost, uint64_t E, const kgpu_mode_opts *opts_in, kgpu_token *tokens, uint64_t token_capacity,
                                  uint64_t *n_tokens, int32_t *cost_out) {
    const char *who = "kgpu_userdict_host";
    using namespace kgpu;
    if (n_tokens) *n_tokens = 0;
    if (!lattice || !conn || !n_tokens || !cost_out || (len && !utf8) || (token_capacity && !tokens)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    const kgpu_mode_opts normal = KGPU_MODE_OPTS_DEFAULT(KGPU_MODE_NORMAL);
    const kgpu_mode_opts opts = opts_in ? *opts_in : normal;
    if (!mode_opts_valid(opts)) { set_error("%s: mode %u is not 0, 1 or 2, or a reserved word is set", who, opts.mode); return KGPU_ERR_INVALID_ARG; }
    const uint64_t N = lattice->n_nodes, NP = lattice->n_positions;
    if (N < 2 || N >= USER_MAX_NODES || !lattice->nodes || !lattice->edge_offsets || !lattice->edge_nodes) {
        set_error("%s: a lattice has BOS, EOS and fewer than 2^32 - 1 nodes", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (len >= (1ull << 31)) { set_error("%s: sentence too long", who); return KGPU_ERR_INVALID_ARG; }
    UserTable table;
    int rc;
    if ((rc = build_user_table(who, keys, key_offsets, left_id, right_id, cost, E, conn_rows, conn_cols, nullptr, nullptr, table))) return rc;
    const UserTableView tv = table.view();
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
    const uint32_t C = (uint32_t)cbyte.size();
    cbyte.push_back((uint32_t)len); kanji.push_back(seen);
    if (E && C && !invoke) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    // (a user node may start at any character and its predecessors are looked up there: the lattice has a position for every character, and EOS's two)
    if (NP < (uint64_t)C + 2) { set_error("%s: the lattice has %llu positions, the text's %u characters need %u", who, (unsigned long long)NP, C, C + 2); return KGPU_ERR_INVALID_ARG; }
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
        if (t > 1 && nd.char_pos < lattice->nodes[t - 1].char_pos) return bad(t, "the nodes are not numbered by start position");
        for (uint32_t e = lattice->edge_offsets[nd.char_pos]; t && e < lattice->edge_offsets[nd.char_pos + 1]; ++e)
            if (lattice->edge_nodes[e] >= t) return bad(t, "a predecessor that is not in front of it");
    }
    // the user nodes, by (q, e): every match of every entry
    struct UNode { uint32_t e, start, end, ids; int32_t cost; };
    std::vector<UNode> un;
    std::vector<uint32_t> ub((size_t)C + 2, 0);   // the user nodes that start at q: [ub[q], ub[q + 1])
    std::vector<uint8_t> hit((size_t)C + 1, 0);
    for (uint32_t q = 0; q < C; ++q) {
        ub[q] = (uint32_t)un.size();
        const uint32_t matches = user_match(tv, utf8, cbyte.data(), C, q, [&](uint32_t g, uint32_t L) {
            const UserGroup gr = tv.groups[g];
            for (uint32_t k = 0; k < gr.count; ++k) un.push_back(UNode{tv.ents[gr.first + k].entry, q, q + L, tv.ents[gr.first + k].ids, tv.ents[gr.first + k].cost});
        });
        // (the groups came shortest key first: by entry now.  The device ranks an entry among the position's other groups instead; the order is the same)
        for (size_t i = ub[q] + 1; i < un.size(); ++i)
            for (size_t k = i; k > ub[q] && un[k - 1].e > un[k].e; --k) std::swap(un[k - 1], un[k]);
        hit[q] = matches != 0;
        if (N + un.size() >= USER_MAX_NODES) { set_error("%s: lattice and user nodes together reach 2^32 - 1", who); return KGPU_ERR_INVALID_ARG; }
    }
    const uint64_t U = un.size();
    ub[C] = ub[(size_t)C + 1] = (uint32_t)U;
    std::vector<std::vector<uint32_t>> uend((size_t)C + 1);   // the user nodes that end at p
    for (uint64_t u = 0; u < U; ++u) uend[un[(size_t)u].end].push_back((uint32_t)u);
    // the state of all N + U nodes; the withdrawn ones first
    std::vector<uint64_t> state((size_t)(N + U), 0);
    std::vector<uint8_t> known_at((size_t)C + 1, 0);
    for (uint64_t t = 1; t + 1 < N; ++t) if (lattice->nodes[t].cls == KGPU_CLASS_KNOWN) known_at[lattice->nodes[t].char_pos] = 1;
    for (uint64_t t = 1; t + 1 < N; ++t) {
        const kgpu_lattice_node &nd = lattice->nodes[t];
        if (nd.cls == KGPU_CLASS_UNKNOWN && nd.char_pos < C && hit[nd.char_pos] && user_withdrawn(hit[nd.char_pos], known_at[nd.char_pos] != 0, invoke[nd.char_pos] != 0)) state[(size_t)t] = USER_WITHDRAWN;
    }
    // the forward, position after position: a predecessor ends where its target starts, so it starts in front of it
    const auto relax = [&](uint64_t t, uint32_t q, uint32_t left, int32_t word) {
        const int16_t *col = conn + (size_t)conn_rows * left;
        uint64_t best = MODE_NONE;
        for (uint32_t e = lattice->edge_offsets[q]; e < lattice->edge_offsets[q + 1]; ++e) {
            const uint32_t j = lattice->edge_nodes[e];
            if (state[j] == USER_WITHDRAWN) continue;
            const uint64_t key = mode_candidate(mode_state_dp(state[j]), j, word, (int32_t)col[(uint16_t)lattice->nodes[j].right_id]);
            if (key < best) best = key;
        }
        if (q <= C)
            for (const uint32_t u : uend[q]) {
                const uint64_t j = N + u;
                const uint64_t key = mode_candidate(mode_state_dp(state[(size_t)j]), (uint32_t)j, word, (int32_t)col[un[u].ids >> 16]);
                if (key < best) best = key;
            }
        state[(size_t)t] = mode_state(best);
    };
    state[0] = mode_bos_state();
    uint64_t t = 1;
    for (uint32_t q = 0; q <= C; ++q) {
        for (; t < N && lattice->nodes[t].char_pos == q; ++t) {
            const kgpu_lattice_node &nd = lattice->nodes[t];
            if (state[(size_t)t] == USER_WITHDRAWN) continue;
            const uint32_t L = nd.end_char - nd.char_pos;
            relax(t, q, (uint16_t)nd.left_id, (int32_t)nd.cost + mode_penalty(opts, nd.cls == KGPU_CLASS_DUMMY, L, kanji[nd.end_char] - kanji[nd.char_pos]));
        }
        for (uint32_t u = ub[q]; u < ub[q + 1]; ++u) {
            const UNode &x = un[u];
            relax(N + u, q, x.ids & 0xFFFFu, x.cost + mode_penalty(opts, false, x.end - x.start, kanji[x.end] - kanji[x.start]));
        }
    }
    if (t != N) return bad(t, "starts behind the text's characters");
    *cost_out = mode_state_dp(state[(size_t)(N - 1)]);
    // the chain from EOS along pre: its head is dropped (a chain's nodes start in front of each other: it ends)
    const auto cls_of = [&](uint64_t node) { return node < N ? lattice->nodes[node].cls : (uint32_t)KGPU_CLASS_USER; };
    const auto span_of = [&](uint64_t node, uint32_t &s, uint32_t &e) {
        if (node < N) { s = lattice->nodes[node].char_pos; e = lattice->nodes[node].end_char; }
        else { s = un[(size_t)(node - N)].start; e = un[(size_t)(node - N)].end; }
    };
    uint64_t T = 0, steps = 0;
    for (uint64_t node = N - 1; mode_state_pre(state[(size_t)node]) != MODE_NO_PRE && steps < N + U; node = mode_state_pre(state[(size_t)node]), ++steps) {
        uint32_t s, e;
        span_of(node, s, e);
        T += mode_record_count(opts.mode, cls_of(node), s, e);
    }
    *n_tokens = T;
    if (T > token_capacity) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)T, (unsigned long long)token_capacity);
        return KGPU_ERR_CAPACITY;
    }
    uint64_t at = T;
    steps = 0;
    for (uint64_t node = N - 1; mode_state_pre(state[(size_t)node]) != MODE_NO_PRE && steps < N + U; node = mode_state_pre(state[(size_t)node]), ++steps) {
        uint32_t s, e;
        span_of(node, s, e);
        const uint32_t cnt = mode_record_count(opts.mode, cls_of(node), s, e);
        at -= cnt;
        if (node >= N) { tokens[at] = user_record(un[(size_t)(node - N)].e, cbyte[s], s, e, cbyte[e] - cbyte[s]); continue; }
        const kgpu_lattice_node &nd = lattice->nodes[node];
        if (cnt == 1) { tokens[at] = nbest_record(nd.cls, nd.id, nd.byte_pos, nd.char_pos, nd.end_char, nd.byte_len); continue; }
        for (uint32_t c = nd.char_pos; c < nd.end_char; ++c) tokens[at + (c - nd.char_pos)] = mode_char_record(nd.id, c, cbyte[c], cbyte[c + 1]);
    }
    return KGPU_OK;
}
