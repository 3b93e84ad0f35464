// tests/c_abi/wordpiece_table_main.cpp -- kanpyo_amd/csrc/kgpu_wordpiece_table.cpp (with kgpu_vocab_table.cpp, whose insert loop it shares) on its own, for a
// sanitizer build: a program with its own main, compiled with those two files by a plain C++ compiler (no HIP, no library).  It builds the tables of a small
// list over a small word table and checks the continuation table, the longest entries, the row entries and the pool; then it splits words held in heap
// copies of exactly their size -- a read past either end is the sanitizer's to report -- and compares every split with a naive restatement of the rule
// written here (std::map, substrings tried longest first): the hand cases, and a few thousand random words over a small alphabet and a random list, with
// the prefixes "##", "" and an 8-byte one.  Prints "wordpiece table ok <words split>".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_internal.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (declared by the header; the table builders report through their `err` string)
}

using namespace kgpu;

static uint32_t rng_state = 2024;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool starts(const std::string &w, size_t i) { return i == 0 || ((unsigned char)w[i] & 0xC0) != 0x80; }

// The rule, naively: maps of the list, every end tried from the longest down.
static std::vector<int32_t> naive(const std::vector<std::string> &list, const std::string &prefix, const std::string &w, uint32_t max_chars, int32_t unk) {
    std::map<std::string, int32_t> initial, cont;
    for (size_t i = 0; i < list.size(); ++i) {
        initial[list[i]] = (int32_t)i;
        if (list[i].size() > prefix.size() && list[i].compare(0, prefix.size(), prefix) == 0) cont[list[i].substr(prefix.size())] = (int32_t)i;
    }
    std::vector<int32_t> out;
    if (w.empty()) return out;
    size_t chars = 0;
    for (size_t i = 0; i < w.size(); ++i) chars += starts(w, i);
    if (chars > max_chars) return {unk};
    size_t start = 0;
    while (start < w.size()) {
        const auto &tb = start == 0 ? initial : cont;
        size_t end = w.size();
        for (; end > start; --end) {
            if (end < w.size() && !starts(w, end)) continue;
            const auto it = tb.find(w.substr(start, end - start));
            if (it != tb.end()) { out.push_back(it->second); break; }
        }
        if (end == start) return {unk};
        start = end;
    }
    return out;
}

static int build(const std::vector<std::string> &list, const std::string &prefix, uint32_t max_chars, int32_t unk, const std::vector<WordRow> &rows, size_t n_known,
                 const std::string &names, const std::string &keys, const uint64_t *key_off, WordpieceTables &t, std::string &err) {
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off{0};
    for (const auto &w : list) { packed.insert(packed.end(), w.begin(), w.end()); off.push_back(packed.size()); }
    std::vector<uint8_t> pf(prefix.begin(), prefix.end());   // (a heap copy of exactly the prefix's size)
    return build_wordpiece_tables(rows.empty() ? nullptr : rows.data(), rows.size(), n_known, (const uint8_t *)names.data(), (const uint8_t *)keys.data(), key_off,
                                  packed.data(), off.data(), list.size(), unk, pf.data(), (uint32_t)pf.size(), max_chars, t, err);
}

static std::vector<int32_t> split(const WordpieceTables &t, const std::string &w, uint32_t max_chars, int32_t unk) {
    std::vector<uint8_t> copy(w.begin(), w.end());
    std::vector<int32_t> out{77};   // (pieces are APPENDED: what is there stays)
    wordpiece_split(t, copy.data(), copy.size(), max_chars, unk, out);
    return std::vector<int32_t>(out.begin() + 1, out.end());
}

int main() {
    const int32_t unk = 0;
    const std::vector<std::string> list = {"[UNK]", "\xe3\x81\x82", "##\xe3\x81\x84", "##\xe3\x81\x86", "##\xe3\x81\x88\xe3\x81\x8a", "##\xe3\x81\x88", "\xe3\x83\x86",
                                           "##\xe3\x82\xb9\xe3\x83\x88", "##abc", "##"};
    const std::string a = "\xe3\x81\x82", i_ = "\xe3\x81\x84", u = "\xe3\x81\x86", e = "\xe3\x81\x88", o = "\xe3\x81\x8a", ka = "\xe3\x81\x8b";
    const std::string tesuto = "\xe3\x83\x86\xe3\x82\xb9\xe3\x83\x88";
    // a word table of four known and two unknown rows: a pool name that splits, one with no split, a known surface row whose key splits in four, a
    // dropped known surface row whose key is the empty word, a pool name listed whole, an unknown surface row (never read)
    const std::string names = tesuto + "absent" + a;
    std::vector<WordRow> rows = {{0, 9}, {9, 6}, {0, WORD_SURFACE}, {0, WORD_SURFACE | WORD_DROPPED}, {15, 3}, {0, WORD_SURFACE}};
    const std::string keys = a + i_ + u + e + o;
    const uint64_t key_off[5] = {0, 0, 0, keys.size(), keys.size()};
    WordpieceTables t;
    std::string err;
    REQUIRE(build(list, "##", 100, unk, rows, 4, names, keys, key_off, t, err) == KGPU_OK);
    REQUIRE(!t.shared && t.cont_words == 6 && t.cont.slots.size() == 16 && t.initial.slots.size() == 32);
    REQUIRE(t.initial_max == 8 && t.cont_max == 6);
    REQUIRE(t.rows.size() == 6 && t.rows[0].count == 2 && t.rows[1].count == 1 && (int32_t)t.rows[1].first == unk && t.rows[2].count == 4 && t.rows[3].count == 0);
    REQUIRE(t.rows[4].count == 1 && t.rows[4].first == 1 && t.rows[5].count == 1 && (int32_t)t.rows[5].first == unk);
    REQUIRE(t.piece_ids.size() == 6 && t.rows[0].first == 0 && t.rows[2].first == 2);
    REQUIRE(t.piece_ids[0] == 6 && t.piece_ids[1] == 7 && t.piece_ids[2] == 1 && t.piece_ids[3] == 2 && t.piece_ids[4] == 3 && t.piece_ids[5] == 4);
    REQUIRE(t.rows_whole == 1 && t.rows_split == 2 && t.rows_unk == 1);
    REQUIRE(vocab_find(t.cont, (const uint8_t *)"abc", 3, -1) == 8 && vocab_find(t.cont, (const uint8_t *)"##abc", 5, -1) == -1 && vocab_find(t.cont, nullptr, 0, -1) == -1);
    size_t n_split = 0;
    std::string long101, long100;
    for (int k = 0; k < 101; ++k) long101 += a;
    for (int k = 0; k < 100; ++k) long100 += a;
    const std::vector<std::string> hand = {a + i_ + u + e + o, a + i_ + u + e, tesuto, "\xe3\x83\x86\xe3\x82\xb9X\xe3\x83\x88", a + i_ + u + e + o + ka, "##abc", "##", "", long101, long100,
                                           "abc", "\xe3\x81", "\x81\x82", std::string("\0", 1)};
    for (const auto &w : hand) {
        REQUIRE(split(t, w, 100, unk) == naive(list, "##", w, 100, unk));
        ++n_split;
    }
    REQUIRE((split(t, hand[0], 100, unk) == std::vector<int32_t>{1, 2, 3, 4}) && (split(t, hand[4], 100, unk) == std::vector<int32_t>{unk}) && split(t, "", 100, unk).empty());
    REQUIRE((split(t, long101, 100, unk) == std::vector<int32_t>{unk}) && (split(t, long100, 100, unk) == std::vector<int32_t>{unk}));   // (## + a is not listed)
    // the same bytes twice: the initial table's error, both indices
    std::vector<std::string> dup = list;
    dup.push_back(list[3]);
    REQUIRE(build(dup, "##", 100, unk, {}, 0, "", "", nullptr, t, err) == KGPU_ERR_INVALID_ARG && err.find(" 3 ") != std::string::npos && err.find(" 10 ") != std::string::npos);
    // bad options
    REQUIRE(build(list, "123456789", 100, unk, {}, 0, "", "", nullptr, t, err) == KGPU_ERR_INVALID_ARG);
    REQUIRE(build(list, "##", 1025, unk, {}, 0, "", "", nullptr, t, err) == KGPU_ERR_INVALID_ARG && build(list, "##", 0, unk, {}, 0, "", "", nullptr, t, err) == KGPU_ERR_INVALID_ARG);
    // no words at all: everything but the empty word is unk
    REQUIRE(build({}, "##", 100, -4, {}, 0, "", "", nullptr, t, err) == KGPU_OK && t.cont.slots.size() == 16 && t.initial_max == 0 && t.cont_max == 0);
    REQUIRE((split(t, "x", 100, -4) == std::vector<int32_t>{-4}) && split(t, "", 100, -4).empty());
    // random words over a small alphabet of 1-, 2-, 3- and 4-byte characters (and a stray continuation byte), a random list, three prefixes
    const std::vector<std::string> alphabet = {"a", "b", "\xc3\xa9", "\xe3\x81\x82", "\xe3\x81\x84", "\xf0\xa0\xae\xb7", "\x82", "#"};
    const auto word_of = [&](size_t chars) { std::string w; for (size_t k = 0; k < chars; ++k) w += alphabet[rnd() % alphabet.size()]; return w; };
    for (const std::string &prefix : {std::string("##"), std::string(""), std::string("12345678")}) {
        std::map<std::string, int> seen;
        std::vector<std::string> rl = {"[UNK]"};
        seen["[UNK]"] = 1;
        for (int k = 0; k < 300; ++k) {
            std::string w = word_of(1 + rnd() % 3);
            if (rnd() % 2) w = prefix + w;
            if (!seen[w]++) rl.push_back(w);
        }
        for (const uint32_t max_chars : {100u, 5u}) {
            REQUIRE(build(rl, prefix, max_chars, unk, {}, 0, "", "", nullptr, t, err) == KGPU_OK);
            REQUIRE(t.shared == prefix.empty() && (t.shared ? t.cont.slots.empty() : !t.cont.slots.empty()));
            size_t multi = 0, unks = 0;
            for (int k = 0; k < 1500; ++k) {
                const std::string w = word_of(rnd() % 9);
                const std::vector<int32_t> got = split(t, w, max_chars, unk);
                REQUIRE(got == naive(rl, prefix, w, max_chars, unk));
                multi += got.size() > 1;
                unks += got.size() == 1 && got[0] == unk;
                ++n_split;
            }
            REQUIRE(multi > 50 && unks > 50);   // (the case is not trivial)
        }
    }
    std::printf("wordpiece table ok %zu\n", n_split);
    return 0;
}
