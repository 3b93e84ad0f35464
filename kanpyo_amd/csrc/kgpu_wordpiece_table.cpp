// kanpyo_amd/csrc/kgpu_wordpiece_table.cpp -- the tables of a WordPiece vocabulary handle (include/kanpyo_gpu.h, "WordPiece ids"; kgpu_wordpiece.hip reads
// them, kgpu_encode_host.cpp uploads them), built once on the host, and the split itself on the host.  HIP-free: a plain C++ compiler builds this file and
// kgpu_vocab_table.cpp alone (tests/c_abi/wordpiece_table_main.cpp).
//
//   initial       build_vocab_table's tables of the whole list, verbatim: what a plain vocabulary has
//   continuation  every list entry that starts with the prefix and is longer than it, the prefix stripped, under the entry's own list index; the same slot
//                 and arena layout, filled by the same insert loop (fill_vocab_table).  prefix_len == 0: it IS the initial table (`shared`), built once.
//   *_max         the longest entry of each table in bytes: no longer prefix of a word can be listed, so neither side probes one
//   rows          one {first, count} per feature row: the row resolved to its bytes as build_vocab_table resolves it and split here, ONCE.  count == 1 keeps
//                 the id inline in `first` (a listed word, or unk_id); count == 0 is the empty word; otherwise the pieces are piece_ids[first .. first + count).
//                 An unknown-class row whose word is the surface is not row-determined: its entry ({unk_id, 1}) is never read.
//   piece_ends    parallel to piece_ids (include/kanpyo_gpu.h, "ids with spans"): where pooled piece k ends inside its row's word, in bytes and in
//                 characters -- wordpiece_split's own ends, kept for the rows whose word is the surface (the dictionary's key); zeros for a feature
//                 column's row, whose pieces all get the token's whole span and never need them.
#include <algorithm>
#include <cstring>

#include "kgpu_internal.h"

namespace kgpu {

namespace {

bool char_start(const uint8_t *p, uint64_t i) { return i == 0 || (p[i] & 0xC0) != 0x80; }

}  // namespace

WordpieceOutcome wordpiece_split(const WordpieceTables &t, const uint8_t *p, uint64_t len, uint32_t max_chars, int32_t unk_id, std::vector<int32_t> &out,
                                 std::vector<PieceEnd> *ends) {
    if (len == 0) return WP_EMPTY;
    uint64_t chars = 0;
    for (uint64_t i = 0; i < len && chars <= max_chars; ++i) chars += char_start(p, i);
    const size_t mark = out.size(), emark = ends ? ends->size() : 0;
    const auto unk = [&]() {   // the WHOLE word is unk_id: its one id ends where the word ends
        out.resize(mark);
        out.push_back(unk_id);
        if (ends) {
            uint64_t all = 0;
            for (uint64_t i = 0; i < len; ++i) all += char_start(p, i);
            ends->resize(emark);
            ends->push_back(PieceEnd{(uint32_t)len, (uint32_t)all});
        }
        return WP_UNK;
    };
    if (chars > max_chars) return unk();
    const int32_t none = -1;   // (list indices are never negative)
    uint64_t start = 0, cstart = 0;   // cstart: the characters in front of `start`
    while (start < len) {
        const VocabTables &tb = start == 0 ? t.initial : t.continuation();
        const uint64_t longest = start == 0 ? t.initial_max : t.continuation_max();
        uint64_t end = len - start < longest ? len : start + longest;
        int32_t id = none;
        for (; end > start; --end) {   // the largest end first: a character start, or the word's end
            if (end < len && !char_start(p, end)) continue;
            if ((id = vocab_find(tb, p + start, end - start, none)) != none) break;
        }
        if (id == none) return unk();   // no piece starts here: the pieces found so far are discarded
        out.push_back(id);
        for (uint64_t i = start; i < end; ++i) cstart += i == start || char_start(p, i);   // (a piece starts at a character start, or at byte 0)
        if (ends) ends->push_back(PieceEnd{(uint32_t)end, (uint32_t)cstart});
        start = end;
    }
    return out.size() - mark == 1 ? WP_WHOLE : WP_SPLIT;
}

int build_wordpiece_tables(const WordRow *rows, size_t n_rows, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off,
                           const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, int32_t unk_id, const uint8_t *prefix, uint32_t prefix_len,
                           uint32_t max_chars, WordpieceTables &out, std::string &err) {
    out = WordpieceTables{};
    if (prefix_len > WORDPIECE_MAX_PREFIX || max_chars == 0 || max_chars > WORDPIECE_MAX_CHARS) { err = "prefix_len above 8, or max_word_chars outside 1..1024"; return KGPU_ERR_INVALID_ARG; }
    if (int rc = build_vocab_table(rows, n_rows, n_known, names, key_bytes, key_off, words, word_offsets, n_words, unk_id, out.initial, err)) return rc;
    for (uint64_t i = 0; i < n_words; ++i) out.initial_max = std::max<uint32_t>(out.initial_max, (uint32_t)(word_offsets[i + 1] - word_offsets[i]));
    out.shared = prefix_len == 0;
    if (out.shared) {
        out.cont_words = n_words;
    } else {
        std::vector<VocabKey> keys;
        for (uint64_t i = 0; i < n_words; ++i) {
            const uint64_t len = word_offsets[i + 1] - word_offsets[i];
            if (len > prefix_len && std::memcmp(words + word_offsets[i], prefix, prefix_len) == 0)
                keys.push_back(VocabKey{words + word_offsets[i] + prefix_len, len - prefix_len, (int32_t)i});
        }
        if (int rc = fill_vocab_table(keys, out.cont, &out.cont_max, err)) return rc;   // (no two can be equal: the list's entries are distinct)
        out.cont_words = keys.size();
    }
    out.rows.assign(n_rows, WordpieceRow{(uint32_t)unk_id, 1});
    std::vector<int32_t> pieces;
    std::vector<PieceEnd> ends;
    for (size_t r = 0; r < n_rows; ++r) {
        const uint8_t *p;
        uint64_t len;
        if (!vocab_row_bytes(rows, r, n_known, names, key_bytes, key_off, p, len)) continue;
        pieces.clear();
        ends.clear();
        const WordpieceOutcome o = wordpiece_split(out, p, len, max_chars, unk_id, pieces, &ends);
        if (o == WP_WHOLE) ++out.rows_whole;
        else if (o == WP_SPLIT) ++out.rows_split;
        else if (o == WP_UNK) ++out.rows_unk;
        if (pieces.size() == 1) { out.rows[r] = WordpieceRow{(uint32_t)pieces[0], 1}; continue; }
        if (out.piece_ids.size() + pieces.size() >= (1ull << 32)) { err = "the rows' pieces take 2^32 ids or more"; return KGPU_ERR_INVALID_ARG; }
        out.rows[r] = WordpieceRow{pieces.empty() ? 0u : (uint32_t)out.piece_ids.size(), (uint32_t)pieces.size()};
        out.piece_ids.insert(out.piece_ids.end(), pieces.begin(), pieces.end());
        if (!(rows[r].len_flags & WORD_SURFACE)) ends.assign(pieces.size(), PieceEnd{0, 0});   // a feature column: whole-token spans, the ends are never read
        out.piece_ends.insert(out.piece_ends.end(), ends.begin(), ends.end());
    }
    return KGPU_OK;
}

}  // namespace kgpu
