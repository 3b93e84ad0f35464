// kanpyo_amd/csrc/kgpu_user_table.cpp -- the table of a user dictionary (include/kanpyo_gpu.h, "user dictionary"; kgpu_user_core.h has its layout and the
// probe): the entries checked, grouped by key, and the distinct keys hashed into an open-addressed table.  HIP-free, compiles alone (with a set_error
// of the caller's): kgpu_userdict_create uploads what this makes, kgpu_userdict_host reads it where it lies.
#include <algorithm>
#include <cstring>

#include "kgpu_internal.h"
#include "kgpu_user_core.h"

namespace kgpu {

// The characters of the len bytes at p, or -1 where they are not UTF-8 (overlong forms, surrogates and values above U+10FFFF are not).
static int64_t utf8_chars(const uint8_t *p, uint64_t len) {
    int64_t chars = 0;
    for (uint64_t b = 0; b < len; ++chars) {
        const uint32_t c = p[b];
        uint32_t l, lo = 0x80u, hi = 0xBFu;
        if (c < 0x80u) l = 1;
        else if (c >= 0xC2u && c <= 0xDFu) l = 2;
        else if (c >= 0xE0u && c <= 0xEFu) { l = 3; if (c == 0xE0u) lo = 0xA0u; if (c == 0xEDu) hi = 0x9Fu; }
        else if (c >= 0xF0u && c <= 0xF4u) { l = 4; if (c == 0xF0u) lo = 0x90u; if (c == 0xF4u) hi = 0x8Fu; }
        else return -1;
        if (b + l > len) return -1;
        for (uint32_t k = 1; k < l; ++k) {
            const uint32_t x = p[b + k];
            if (k == 1 ? (x < lo || x > hi) : ((x & 0xC0u) != 0x80u)) return -1;
        }
        b += l;
    }
    return chars;
}

UserTableView UserTable::view() const {
    return UserTableView{slots.data(), slots.empty() ? 0u : (uint32_t)slots.size() - 1u, groups.data(), ents.data(), arena.data(), len_mask,
                         (uint32_t)ents.size(), (uint32_t)groups.size()};
}

int build_user_table(const char *who, const uint8_t *keys, const uint64_t *key_offsets, const uint16_t *left_id, const uint16_t *right_id, const int16_t *cost,
                     uint64_t E, uint64_t conn_rows, uint64_t conn_cols, const std::vector<uint32_t> *left_rank, const std::vector<uint32_t> *right_rank,
                     UserTable &out) {
    out = UserTable{};
    if (!E) return KGPU_OK;
    if (!keys || !key_offsets || !left_id || !right_id || !cost) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (E >= (1ull << 31)) { set_error("%s: %llu entries: fewer than 2^31 are taken", who, (unsigned long long)E); return KGPU_ERR_INVALID_ARG; }
    if (key_offsets[0] != 0) { set_error("%s: key_offsets[0] is not 0", who); return KGPU_ERR_INVALID_ARG; }
    const auto bad = [&](uint64_t e, const char *what) { set_error("%s: entry %llu: %s", who, (unsigned long long)e, what); return KGPU_ERR_INVALID_ARG; };
    for (uint64_t e = 0; e < E; ++e) {
        if (key_offsets[e + 1] < key_offsets[e]) return bad(e, "key offsets run backwards");
        const uint64_t len = key_offsets[e + 1] - key_offsets[e];
        if (!len) return bad(e, "an empty key");
        if (len > USER_MAX_KEY_BYTES) return bad(e, "a key of more than 255 bytes");
        const int64_t chars = utf8_chars(keys + key_offsets[e], len);
        if (chars < 0) return bad(e, "a key that is not UTF-8");
        if (chars > (int64_t)USER_MAX_KEY_CHARS) return bad(e, "a key of more than 64 characters");
        if (left_id[e] >= conn_cols || right_id[e] >= conn_rows) return bad(e, "a context id outside the matrix");
        out.len_mask |= 1ull << (chars - 1);
        out.longest = std::max(out.longest, (uint32_t)chars);
    }
    // the entries by (key bytes, e): a group per distinct key, its entries in ascending e
    std::vector<uint32_t> order((size_t)E);
    for (uint64_t e = 0; e < E; ++e) order[(size_t)e] = (uint32_t)e;
    const auto key_of = [&](uint32_t e, uint64_t &len) { len = key_offsets[e + 1] - key_offsets[e]; return keys + key_offsets[e]; };
    const auto cmp = [&](uint32_t a, uint32_t b) {
        uint64_t la, lb;
        const uint8_t *pa = key_of(a, la), *pb = key_of(b, lb);
        const int c = std::memcmp(pa, pb, (size_t)std::min(la, lb));
        return c != 0 ? c : la < lb ? -1 : la > lb ? 1 : 0;
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { const int c = cmp(a, b); return c != 0 ? c < 0 : a < b; });
    out.ents.resize((size_t)E);
    for (uint64_t i = 0; i < E; ++i) {
        const uint32_t e = order[(size_t)i];
        if (!i || cmp(order[(size_t)i - 1], e) != 0) {
            uint64_t len;
            const uint8_t *p = key_of(e, len);
            out.groups.push_back(UserGroup{(uint32_t)out.arena.size(), (uint32_t)len, (uint32_t)i, 0});
            out.arena.insert(out.arena.end(), p, p + len);
        }
        out.groups.back().count++;
        const uint32_t l = left_rank && !left_rank->empty() ? (*left_rank)[left_id[e]] : left_id[e], r = right_rank && !right_rank->empty() ? (*right_rank)[right_id[e]] : right_id[e];
        out.ents[(size_t)i] = UserEntry{e, l | (r << 16), (int32_t)cost[e], 0};
    }
    out.arena.resize((out.arena.size() + 15) & ~(size_t)15, 0);
    size_t slots = 16;
    while (slots < 2 * out.groups.size()) slots <<= 1;
    out.slots.assign(slots, 0);
    for (size_t g = 0; g < out.groups.size(); ++g) {
        const uint32_t h = user_key_hash(out.arena.data() + out.groups[g].key_off, out.groups[g].key_bytes);
        size_t at = h & (slots - 1);
        while (out.slots[at]) at = (at + 1) & (slots - 1);
        out.slots[at] = user_slot_tag(h, (uint32_t)g);
    }
    return KGPU_OK;
}

}  // namespace kgpu

// (tests) the hash of a key and the slot count of a table of `groups` distinct keys: what tests/table_keys.py needs to build colliding and crowded keys
extern "C" uint32_t kgpu_debug_userdict_hash(const uint8_t *p, uint32_t len) { return kgpu::user_key_hash(p, len); }
extern "C" uint64_t kgpu_debug_userdict_slots(uint64_t groups) {
    uint64_t slots = 16;
    while (slots < 2 * groups) slots <<= 1;
    return slots;
}
