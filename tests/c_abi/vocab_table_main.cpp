// tests/c_abi/vocab_table_main.cpp -- kanpyo_amd/csrc/kgpu_vocab_table.cpp on its own, for a sanitizer build: a program with its own main, compiled
// together with that one file by a plain C++ compiler (no HIP, no library).  It builds the tables of a few thousand words of lengths 0..3072 over a
// small word table, probes every word, near misses of every word and the rows, and checks the duplicate error.  Then keys chosen against the table
// (tests/table_keys.py found them; they are data here): different words with one full 32-bit hash, and eight words whose home is the last of 16 slots.
// Prints "vocab table ok <words>".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_internal.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (declared by the header; the table builder reports through its `err` string)
}

using namespace kgpu;

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// A table of these words alone, over no rows.
static int build_words(const std::vector<std::string> &words, int32_t unk, VocabTables &t, std::string &err) {
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off{0};
    for (const auto &w : words) { packed.insert(packed.end(), w.begin(), w.end()); off.push_back(packed.size()); }
    return build_vocab_table(nullptr, 0, 0, nullptr, nullptr, nullptr, packed.data(), off.data(), words.size(), unk, t, err);
}
static int32_t find(const VocabTables &t, const std::string &w, int32_t unk) {
    std::vector<uint8_t> copy(w.begin(), w.end());   // (a heap copy of exactly the word's size)
    return vocab_find(t, copy.data(), copy.size(), unk);
}
static uint32_t hash_of(const std::string &w) { return vocab_key_hash((const uint8_t *)w.data(), w.size()); }

int main() {
    std::vector<std::string> words;
    words.push_back("");   // the empty word is a legal entry
    words.push_back("pool-name");
    const int lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 3071, 3072};
    for (int L : lens)
        for (int k = 0; k < 3; ++k) {
            std::string w((size_t)L, '\0');
            for (auto &c : w) c = (char)(rnd() & 0xFF);
            w[(size_t)L - 1] = (char)k;   // (distinct within the length: they differ in the last byte)
            words.push_back(w);
        }
    for (int i = 0; i < 4000; ++i) {   // distinct by their decimal head
        std::string w = std::to_string(i) + ":";
        const size_t extra = rnd() % 24;
        for (size_t k = 0; k < extra; ++k) w.push_back((char)(rnd() & 0xFF));
        words.push_back(w);
    }
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off{0};
    for (const auto &w : words) { packed.insert(packed.end(), w.begin(), w.end()); off.push_back(packed.size()); }
    // a word table of four known and two unknown rows: a pool name that is listed, one that is not, a known surface row, a dropped known surface
    // row whose key is the empty word, and an unknown surface row
    const std::string names = "pool-nameabsent-name";
    std::vector<WordRow> rows = {{0, 9}, {9, 11}, {0, WORD_SURFACE}, {0, WORD_SURFACE | WORD_DROPPED}, {0, 9}, {0, WORD_SURFACE}};
    const std::string keys = words[30];
    const uint64_t key_off[5] = {0, 0, 0, keys.size(), keys.size()};
    VocabTables t;
    std::string err;
    const int32_t unk = -5;
    REQUIRE(build_vocab_table(rows.data(), rows.size(), 4, (const uint8_t *)names.data(), (const uint8_t *)keys.data(), key_off, packed.data(), off.data(),
                              words.size(), unk, t, err) == KGPU_OK);
    REQUIRE(t.slots.size() >= 2 * words.size() && (t.slots.size() & (t.slots.size() - 1)) == 0);
    REQUIRE(t.row_id.size() == 6 && t.row_id[0] == 1 && t.row_id[1] == unk && t.row_id[2] == 30 && t.row_id[3] == 0 && t.row_id[4] == 1 && t.row_id[5] == unk);
    REQUIRE(t.rows_resolved == 4);
    for (size_t i = 0; i < words.size(); ++i) {
        const std::string &w = words[i];
        REQUIRE(vocab_find(t, (const uint8_t *)w.data(), w.size(), unk) == (int32_t)i);
        // heap copies of exactly the word's size: a read past either end is the sanitizer's to report
        std::vector<uint8_t> longer(w.begin(), w.end());
        longer.push_back(0);
        const int32_t a = vocab_find(t, longer.data(), longer.size(), unk);
        REQUIRE(a == unk || words[(size_t)a] == std::string(longer.begin(), longer.end()));
        if (!w.empty()) {
            std::vector<uint8_t> flipped(w.begin(), w.end());
            flipped.back() ^= 0x80;
            const int32_t f = vocab_find(t, flipped.data(), flipped.size(), unk);
            REQUIRE(f == unk || words[(size_t)f] == std::string(flipped.begin(), flipped.end()));
            std::vector<uint8_t> shorter(w.begin(), w.end() - 1);
            const int32_t s = vocab_find(t, shorter.data(), shorter.size(), unk);
            REQUIRE(s == unk || words[(size_t)s] == std::string(shorter.begin(), shorter.end()));
        }
    }
    // the same bytes twice: an error that names both indices
    std::vector<uint8_t> p2 = packed;
    std::vector<uint64_t> o2 = off;
    p2.insert(p2.end(), words[17].begin(), words[17].end());
    o2.push_back(p2.size());
    REQUIRE(build_vocab_table(rows.data(), rows.size(), 4, (const uint8_t *)names.data(), (const uint8_t *)keys.data(), key_off, p2.data(), o2.data(),
                              words.size() + 1, unk, t, err) == KGPU_ERR_INVALID_ARG);
    REQUIRE(err.find(" 17 ") != std::string::npos && err.find(std::to_string(words.size())) != std::string::npos);
    // no words at all: 16 free slots, everything is unk
    REQUIRE(build_vocab_table(rows.data(), rows.size(), 4, (const uint8_t *)names.data(), (const uint8_t *)keys.data(), key_off, nullptr, nullptr, 0, unk, t, err) == KGPU_OK);
    REQUIRE(t.slots.size() == 16 && t.rows_resolved == 0 && vocab_find(t, nullptr, 0, unk) == unk);
    // different words with one hash: two of 5 bytes, two of 8, two of 21 that differ in their first 5 bytes only, two of 8 that share home slot 63 of 64,
    // 8 bytes against 7, 16 against 9.  Only the compare with the arena entry tells them apart.
    struct Key { const char *p; size_t n; };
    const Key pairs[][2] = {
        {{"\065\043\051\345\006", 5}, {"\221\253\112\165\021", 5}},
        {{"\005\362\041\335\112\153\122\115", 8}, {"\042\131\256\007\313\074\216\154", 8}},
        {{"\335\320\131\300\172\213\112\345\361\251\101\006\240\225\152\046\257\274\315\257\345", 21}, {"\077\220\327\017\213\213\112\345\361\251\101\006\240\225\152\046\257\274\315\257\345", 21}},
        {{"\375\210\073\061\101\374\175\120", 8}, {"\350\217\076\303\302\374\175\120", 8}},
        {{"\142\145\247\363\301\174\333\035", 8}, {"\104\247\004\176\375\244\117", 7}},
        {{"\300\065\312\131\123\006\166\345\122\132\204\147\250\250\142\340", 16}, {"\016\344\147\122\127\056\321\161\232", 9}},
    };
    const size_t n_pairs = sizeof pairs / sizeof pairs[0];
    std::vector<std::string> both, first, second;
    for (const auto &pr : pairs) {
        const std::string a(pr[0].p, pr[0].n), b(pr[1].p, pr[1].n);
        REQUIRE(a != b && hash_of(a) == hash_of(b));   // (the data is what it claims to be)
        both.push_back(a); both.push_back(b);
        first.push_back(a); second.push_back(b);
    }
    REQUIRE(build_words(both, unk, t, err) == KGPU_OK && t.slots.size() == 32);
    for (size_t i = 0; i < both.size(); ++i) REQUIRE(find(t, both[i], unk) == (int32_t)i);
    REQUIRE(build_words(first, unk, t, err) == KGPU_OK);
    for (size_t i = 0; i < n_pairs; ++i) REQUIRE(find(t, first[i], unk) == (int32_t)i && find(t, second[i], unk) == unk);   // the partner of a word listed alone
    REQUIRE(build_words(second, unk, t, err) == KGPU_OK);
    for (size_t i = 0; i < n_pairs; ++i) REQUIRE(find(t, second[i], unk) == (int32_t)i && find(t, first[i], unk) == unk);
    both.push_back(both[3]);   // the same bytes twice among them: still the duplicate error
    REQUIRE(build_words(both, unk, t, err) == KGPU_ERR_INVALID_ARG && err.find(" 3 ") != std::string::npos && err.find(" 12 ") != std::string::npos);
    // eight words of home slot 15 of 16: the chain is slot 15, then 0..6; an absent key of home 15 walks all of it, one of home 3 the rest of it
    const char *cluster[] = {"\063\110\337\112\275\164", "\202\113\300\040\144\316", "\323\162\251\200\147\053", "\152\033\030\325\212\051",
                             "\262\200\276\353\350\263", "\365\061\044\013\237\244", "\122\312\315\356\137\047", "\052\233\067\033\220\006"};
    const std::string absent15 = "\342\047\302\103\310\337", absent3 = "\141\062\314\044\174\357";
    std::vector<std::string> chain(cluster, cluster + 8);
    for (const auto &w : chain) REQUIRE(w.size() == 6 && (hash_of(w) & 15) == 15);
    REQUIRE((hash_of(absent15) & 15) == 15 && (hash_of(absent3) & 15) == 3);
    REQUIRE(build_words(chain, unk, t, err) == KGPU_OK && t.slots.size() == 16);
    REQUIRE(t.slots[15].tag != 0 && t.slots[15].id == 0 && t.slots[7].tag == 0);
    for (size_t i = 1; i < 8; ++i) REQUIRE(t.slots[i - 1].tag != 0 && t.slots[i - 1].id == (int32_t)i);
    for (size_t i = 0; i < 8; ++i) REQUIRE(find(t, chain[i], unk) == (int32_t)i);
    REQUIRE(find(t, absent15, unk) == unk && find(t, absent3, unk) == unk);
    std::printf("vocab table ok %zu\n", words.size());
    return 0;
}
