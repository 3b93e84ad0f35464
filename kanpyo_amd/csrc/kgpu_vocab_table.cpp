// kanpyo_amd/csrc/kgpu_vocab_table.cpp -- the two tables of a vocabulary handle (include/kanpyo_gpu.h, "vocabulary ids"; kgpu_encode.hip reads them,
// kgpu_encode_host.cpp uploads them), built once on the host.  HIP-free: a plain C++ compiler builds this file alone (tests/c_abi/vocab_table_main.cpp).
//
//   row_id   one int32 per feature row: the row resolved to its word's bytes exactly as the counts read-out resolves it -- the pool name when the row's
//            entry is not a surface row, the dictionary's key of the id for a known row whose word is its surface -- and those bytes looked up in the
//            list; a miss stores unk_id.  An unknown-class row whose word is the surface is not row-determined: its entry is never read.
//   slots    the frozen byte-keyed table, the counts table's layout: a power of two of {tag, id} slots, at least twice the list and at least 16 (load
//            <= 0.5: probe chains stay short, a free slot always ends a probe), tag = hash << 32 | (arena entry / 8 + 1), linear probing from hash & mask.
//   arena    entries of {u32 length, u32 hash, the bytes padded to 8}.  ALL list words go in: a row-determined word costs a slot and hurts nothing.
#include <cstring>

#include "kgpu_internal.h"

namespace kgpu {

// FNV-1a over the bytes, then murmur3's finaliser with the length folded in: key_hash of kgpu_records_dev.h, restated.
uint32_t vocab_key_hash(const uint8_t *p, uint64_t len) {
    uint32_t h = 2166136261u;
    for (uint64_t i = 0; i < len; ++i) h = (h ^ p[i]) * 16777619u;
    h ^= (uint32_t)len;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

namespace {

// The slot of these bytes, or the free slot that ends their probe (the table is never full: load <= 0.5).
size_t probe(const VocabTables &t, uint32_t h, const uint8_t *p, uint64_t len, bool &found) {
    const size_t mask = t.slots.size() - 1;
    size_t i = h & mask;
    for (size_t n = 0; n <= mask; ++n, i = (i + 1) & mask) {
        const VocabSlot &s = t.slots[i];
        if (s.tag == 0) { found = false; return i; }
        if ((uint32_t)(s.tag >> 32) != h) continue;
        const uint8_t *e = t.arena.data() + ((s.tag & 0xFFFFFFFFull) - 1) * 8;
        uint32_t elen;
        std::memcpy(&elen, e, 4);
        if (elen == len && (len == 0 || std::memcmp(e + COUNT_ENTRY_HEAD, p, (size_t)len) == 0)) { found = true; return i; }
    }
    found = false;
    return mask + 1;   // (unreachable while the load is <= 0.5)
}

}  // namespace

int32_t vocab_find(const VocabTables &t, const uint8_t *p, uint64_t len, int32_t unk) {
    if (t.slots.empty() || len >= (1ull << 32)) return unk;
    bool found;
    const size_t i = probe(t, vocab_key_hash(p, len), p, len, found);
    return found ? t.slots[i].id : unk;
}

int fill_vocab_table(const std::vector<VocabKey> &keys, VocabTables &out, uint32_t *max_len, std::string &err) {
    uint64_t arena_bytes = 0;
    for (const VocabKey &k : keys) arena_bytes += COUNT_ENTRY_HEAD + ((k.len + 7) & ~7ull);
    if (arena_bytes / 8 + 1 >= (1ull << 32)) { err = "the words take 32 GiB of key arena or more"; return KGPU_ERR_INVALID_ARG; }
    size_t slots = 16;
    while (slots < 2 * keys.size()) slots <<= 1;
    out.slots.assign(slots, VocabSlot{0, 0, {0, 0}});
    out.arena.assign((size_t)arena_bytes + 16, 0);   // (16 spare bytes: the device reads whole 8-byte words of an entry, never past its padding)
    uint64_t at = 0;
    uint32_t longest = 0;
    for (const VocabKey &k : keys) {
        const uint64_t len = k.len;
        const uint8_t *p = len ? k.p : nullptr;
        const uint32_t h = vocab_key_hash(p, len);
        bool found;
        const size_t slot = probe(out, h, p, len, found);
        if (found) {
            err = "words " + std::to_string(out.slots[slot].id) + " and " + std::to_string(k.id) + " of the list are the same bytes";
            return KGPU_ERR_INVALID_ARG;
        }
        uint8_t *e = out.arena.data() + at;
        const uint32_t len32 = (uint32_t)len;
        std::memcpy(e, &len32, 4);
        std::memcpy(e + 4, &h, 4);
        if (len) std::memcpy(e + COUNT_ENTRY_HEAD, p, (size_t)len);
        out.slots[slot].tag = ((unsigned long long)h << 32) | (at / 8 + 1);
        out.slots[slot].id = k.id;
        at += COUNT_ENTRY_HEAD + ((len + 7) & ~7ull);
        if (len32 > longest) longest = len32;
    }
    if (max_len) *max_len = longest;
    return KGPU_OK;
}

// The way back (include/kanpyo_gpu.h, "text from ids"): every slot names its id and its arena entry, so one pass over the slots gives entry[id] = the
// entry's offset / 8.  The list's words are distinct and all listed: every id below n_words is met exactly once.
void build_decode_entries(const VocabTables &t, uint64_t n_words, std::vector<uint32_t> &entry) {
    entry.assign((size_t)n_words, 0);
    for (const VocabSlot &s : t.slots)
        if (s.tag != 0 && s.id >= 0 && (uint64_t)s.id < n_words) entry[(size_t)s.id] = (uint32_t)(s.tag & 0xFFFFFFFFull) - 1;
}

bool vocab_row_bytes(const WordRow *rows, size_t r, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off, const uint8_t *&p, uint64_t &len) {
    const WordRow &row = rows[r];
    if (!(row.len_flags & WORD_SURFACE)) { p = names + row.off; len = row.len_flags & WORD_LEN_MASK; return true; }
    if (r < n_known && key_off) { p = key_bytes + key_off[r]; len = key_off[r + 1] - key_off[r]; return true; }
    return false;   // an unknown row whose word is the surface: looked up by its bytes, token by token
}

int build_vocab_table(const WordRow *rows, size_t n_rows, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off,
                      const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, int32_t unk_id, VocabTables &out, std::string &err) {
    out = VocabTables{};
    if (n_words > 0x7FFFFFFFull) { err = "more than 2^31 - 1 words"; return KGPU_ERR_INVALID_ARG; }
    if (n_words && !word_offsets) { err = "words without offsets"; return KGPU_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n_words; ++i) {
        if (word_offsets[i + 1] < word_offsets[i]) { err = "word offsets run backwards at " + std::to_string(i); return KGPU_ERR_INVALID_ARG; }
        const uint64_t len = word_offsets[i + 1] - word_offsets[i];
        if (len >= (1ull << 30)) { err = "word " + std::to_string(i) + " has 2^30 bytes or more"; return KGPU_ERR_INVALID_ARG; }
    }
    if (n_words && word_offsets[n_words] != word_offsets[0] && !words) { err = "word offsets without words"; return KGPU_ERR_INVALID_ARG; }
    std::vector<VocabKey> keys((size_t)n_words);
    for (uint64_t i = 0; i < n_words; ++i) {
        const uint64_t len = word_offsets[i + 1] - word_offsets[i];
        keys[(size_t)i] = VocabKey{len ? words + word_offsets[i] : nullptr, len, (int32_t)i};
    }
    if (int rc = fill_vocab_table(keys, out, nullptr, err)) return rc;
    out.row_id.assign(n_rows, unk_id);
    for (size_t r = 0; r < n_rows; ++r) {
        const uint8_t *p;
        uint64_t len;
        if (!vocab_row_bytes(rows, r, n_known, names, key_bytes, key_off, p, len)) continue;
        const int32_t none = -1;   // (list indices are never negative)
        const int32_t id = vocab_find(out, len ? p : nullptr, len, none);
        if (id != none) { out.row_id[r] = id; ++out.rows_resolved; }
    }
    return KGPU_OK;
}

}  // namespace kgpu
