// kanpyo_amd/csrc/kgpu_user_batch.cpp -- the user dictionary's handle (kgpu_userdict_create / _destroy / _get_info) and kgpu_tokenize_batch_user: the decode
// of n sentences in host memory over their lattices widened by the handle's matches (include/kanpyo_gpu.h, "user dictionary").
//
// A kept-lattice call (kgpu_lattice_call.h has the protocol; DESIGN.md, "The kept-lattice protocol"): this file has the call's own part -- the launches of
// kgpu_user.hip over a chunk's lattices, the slab they keep behind them, and where the records and costs go.
#include "kgpu_lattice_call.h"
#include "kgpu_user_core.h"

extern "C" int kgpu_userdict_create(kgpu_dict *d, const uint8_t *keys, const uint64_t *key_offsets, const uint16_t *left_id, const uint16_t *right_id,
                                    const int16_t *cost, uint64_t E, kgpu_userdict **out) {
    const char *who = "kgpu_userdict_create";
    if (out) *out = nullptr;
    if (!d || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    // the device matrix is addressed by ranked ids: the dictionary's own id -> its rank (kgpu_dict.cpp keeps the way back)
    const auto inverse = [](const std::vector<uint32_t> &of_rank) {
        std::vector<uint32_t> rank(of_rank.size());
        for (uint32_t r = 0; r < of_rank.size(); ++r) rank[of_rank[r]] = r;
        return rank;
    };
    const std::vector<uint32_t> left_rank = inverse(d->left_of_rank), right_rank = inverse(d->right_of_rank);
    UserTable t;
    int rc;
    if ((rc = build_user_table(who, keys, key_offsets, left_id, right_id, cost, E, d->info.conn_rows, d->info.conn_cols, &left_rank, &right_rank, t))) return rc;
    const size_t slot_bytes = t.slots.size() * 8, group_bytes = t.groups.size() * sizeof(UserGroup), ent_bytes = t.ents.size() * sizeof(UserEntry);
    const size_t total = slot_bytes + group_bytes + ent_bytes + t.arena.size();   // (every part a multiple of 16 bytes)
    if (total) HIPCHECK(hipSetDevice(d->device));   // (ahead of the handle: nothing to give back on this path)
    kgpu_userdict *u = new kgpu_userdict();
    u->info.entries = E; u->info.keys = t.groups.size(); u->info.longest_key = t.longest; u->info.device_bytes = total;
    if (total) {
        std::vector<uint8_t> block(total);
        std::memcpy(block.data(), t.slots.data(), slot_bytes);
        std::memcpy(block.data() + slot_bytes, t.groups.data(), group_bytes);
        std::memcpy(block.data() + slot_bytes + group_bytes, t.ents.data(), ent_bytes);
        std::memcpy(block.data() + slot_bytes + group_bytes + ent_bytes, t.arena.data(), t.arena.size());
        hipError_t e;
        if ((e = hipMalloc(&u->d_block, total)) != hipSuccess || (e = hipMemcpy(u->d_block, block.data(), total, hipMemcpyHostToDevice)) != hipSuccess) {
            if (u->d_block) (void)hipFree(u->d_block);
            delete u;
            set_error("%s: %zu bytes of device memory: %s", who, total, hipGetErrorString(e));
            return KGPU_ERR_HIP;
        }
        const uint8_t *p = (const uint8_t *)u->d_block;
        u->view = UserTableView{(const uint64_t *)p, (uint32_t)t.slots.size() - 1u, (const UserGroup *)(p + slot_bytes), (const UserEntry *)(p + slot_bytes + group_bytes),
                                p + slot_bytes + group_bytes + ent_bytes, t.len_mask, (uint32_t)t.ents.size(), (uint32_t)t.groups.size()};
    }
    u->dict = d;
    d->refs.fetch_add(1, std::memory_order_relaxed);
    *out = u;
    return KGPU_OK;
}

extern "C" void kgpu_userdict_destroy(kgpu_userdict *u) {
    if (!u) return;
    (void)hipSetDevice(u->dict->device);
    if (u->d_block) (void)hipFree(u->d_block);
    dict_release(u->dict);
    delete u;
}

extern "C" int kgpu_userdict_get_info(const kgpu_userdict *u, kgpu_userdict_info *info) {
    if (!u || !info) { set_error("kgpu_userdict_get_info: null argument"); return KGPU_ERR_INVALID_ARG; }
    *info = u->info;
    return KGPU_OK;
}

namespace {

struct UserOps : LatticeOps {
    const char *who = "kgpu_tokenize_batch_user";
    static constexpr LatticeHook hook = HOOK_USER;
    static constexpr const char *measure_what = "forward launch";
    const kgpu_userdict *u;
    kgpu_mode_opts opts;
    kgpu_token *tokens; uint64_t token_capacity;
    uint64_t *tok_offsets; int32_t *costs;
    uint64_t *n_tokens;
    UserArgs ua{};
    std::vector<uint64_t> toff;

    void begin() { tok_offsets[0] = 0; }
    // the scan's array with the costs behind it: sent_len [m + 1] | costs [m] (int32)
    size_t chunk_words(uint64_t m) const { return (size_t)(m + 1 + (m + 1) / 2 + 1); }
    void fill(const LatticeChunk &f) {
        ua = UserArgs{};
        ModeArgs &g = ua.m;
        g.n = f.m; g.opts = opts; g.ctl = f.ctl; g.arena = f.arena; g.arena_bytes = f.arena_bytes; g.utf8 = f.utf8; g.offsets = f.offsets; g.desc = f.desc;
        g.conn = f.conn; g.conn_rows = f.conn_rows; g.status = f.status;
        g.sent_len = f.words; g.costs = (int32_t *)(g.sent_len + f.m + 1);
        const DictView &v = u->dict->view;
        ua.t = u->view; ua.cat = v.cat; ua.cat_len = v.cat_len; ua.cinfo = v.cinfo;
    }
    int measure(hipStream_t st) { return launch_user_measure(ua, st); }
    void totals(const uint64_t *t[2]) const { t[0] = ua.m.sent_len + ua.m.n; }   // the chunk's records
    bool fits(const uint64_t done[2], const uint64_t sz[2]) const { return done[0] + sz[0] <= token_capacity; }
    size_t out_bytes(const uint64_t sz[2]) const { return (size_t)sz[0] * sizeof(kgpu_token); }
    void place(uint8_t *blk, const uint64_t sz[2]) { ua.m.tokens = (kgpu_token *)blk; ua.m.token_cap = sz[0]; }
    int write(hipStream_t st) { return launch_user_write(ua, st); }
    // (tok_offsets and costs are delivered whether or not the records fit, as kgpu_tokenize_batch_mode delivers them)
    hipError_t deliver(const LatticeChunk &f, const uint64_t done[2], const uint64_t sz[2], bool fits, const char *&what) {
        hipError_t e;
        what = "D2H records";
        if (fits && (e = d2h(tokens + done[0], ua.m.tokens, (size_t)sz[0] * sizeof(kgpu_token), f.stream)) != hipSuccess) return e;
        toff.resize((size_t)f.m + 1);
        what = "D2H offsets";
        if ((e = d2h(toff.data(), ua.m.sent_len, (size_t)(f.m + 1) * 8, f.stream)) != hipSuccess) return e;
        what = "D2H costs";
        return costs ? d2h(costs + f.lo, ua.m.costs, (size_t)f.m * 4, f.stream) : hipSuccess;
    }
    void fix_up(const LatticeChunk &f, const uint64_t done[2], const uint64_t *, bool) {
        for (uint64_t i = 0; i <= f.m; ++i) tok_offsets[f.lo + i] = done[0] + toff[(size_t)i];
    }
    void report(const uint64_t done[2]) { *n_tokens = done[0]; }
    void too_small(const uint64_t done[2]) {
        set_error("buffers too small: need %llu tokens (capacity %llu)", (unsigned long long)done[0], (unsigned long long)token_capacity);
    }
};

}  // namespace

extern "C" int kgpu_tokenize_batch_user(kgpu_dict *d, const kgpu_userdict *u, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_mode_opts *opts,
                                        kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs, uint8_t *status, uint64_t *n_tokens) {
    UserOps ops;
    const char *who = ops.who;
    if (n_tokens) *n_tokens = 0;
    if (!d || !u || !offsets || !tok_offsets || !n_tokens || (token_capacity && !tokens)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if (u->dict != d) { set_error("%s: the user dictionary was made over another dictionary", who); return KGPU_ERR_INVALID_ARG; }
    const kgpu_mode_opts normal = KGPU_MODE_OPTS_DEFAULT(KGPU_MODE_NORMAL);
    ops.opts = opts ? *opts : normal;
    if (!kgpu::mode_opts_valid(ops.opts)) { set_error("%s: mode %u is not 0, 1 or 2, or a reserved word is set", who, ops.opts.mode); return KGPU_ERR_INVALID_ARG; }
    ops.u = u; ops.tokens = tokens; ops.token_capacity = token_capacity; ops.tok_offsets = tok_offsets; ops.costs = costs; ops.n_tokens = n_tokens;
    return lattice_call(ops, d, utf8, offsets, n, status);
}
