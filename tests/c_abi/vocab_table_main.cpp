// tests/c_abi/vocab_table_main.cpp -- kanpyo_amd/csrc/kgpu_vocab_table.cpp on its own, for a sanitizer build: a program with its own main, compiled
// together with that one file by a plain C++ compiler (no HIP, no library).  It builds the tables of a few thousand words of lengths 0..3072 over a
// small word table, probes every word, near misses of every word and the rows, and checks the duplicate error.  Prints "vocab table ok <words>".
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
    std::printf("vocab table ok %zu\n", words.size());
    return 0;
}
