// tests/c_abi/decode_sanitize.cpp -- the host side of the text from ids (include/kanpyo_gpu.h, "text from ids"), compiled beside this file without HIP
// (kanpyo_amd/csrc/kgpu_decode_host.cpp, kgpu_vocab_table.cpp) with every buffer allocated at its exact size: built with -fsanitize=address,undefined
// and run as it is, a read or a store one element outside any array ends the program.  Two parts:
//   the id -> entry table (build_decode_entries over build_vocab_table's tables): entry[id] names an arena entry that holds word id's length and bytes;
//   kgpu_decode_host against a naive restatement of rules 1 to 3 on std::string, ragged and padded, with the capacity protocol (one byte short:
//   nothing is written; the exact size: nothing beyond it).
// Prints "decode sanitized ok <calls> <tables>".
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_internal.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (the library's writes a thread-local message)
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "decode_sanitize: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

// A list of n distinct words: the empty word, the prefix, a doubled prefix, the lengths at which a load or a unit changes, bytes that are not UTF-8.
static std::vector<std::string> make_list(size_t n, const std::string &prefix) {
    std::vector<std::string> out;
    const auto add = [&](const std::string &w) {
        for (const std::string &o : out) if (o == w) return;
        if (out.size() < n) out.push_back(w);
    };
    const size_t lens[] = {1, 7, 8, 9, 64, 65, 3072};
    add(""); add(prefix); add(prefix + prefix + "y"); add("\xff\xfe"); add(prefix + "ab");
    for (size_t len : lens) { std::string w(len, 'a'); for (char &ch : w) ch = (char)rnd(); add(w); }
    while (out.size() < n) {
        std::string w = (rnd() % 3 == 0) ? prefix : std::string();
        for (uint32_t k = 1 + rnd() % 10; k; --k) w.push_back((char)('a' + rnd() % 26));
        add(w);
    }
    for (size_t i = out.size(); i > 1; --i) std::swap(out[i - 1], out[rnd() % i]);
    return out;
}

static bool skipped(const kgpu_decode_opts &o, int32_t id) {
    for (uint32_t i = 0; i < o.n_skip; ++i) if (o.skip_ids[i] == id) return true;
    return false;
}

int main() {
    uint64_t calls = 0, tables = 0;
    const std::string prefixes[] = {"", "##", "@@cont@@"};
    const std::string seps[] = {"", " ", "\xe3\x80\x80", "<--sep->"};
    const size_t sizes[] = {1, 2, 3, 17, 40, 200};
    for (int round = 0; round < 180; ++round) {
        const std::string &prefix = prefixes[round % 3];
        const std::vector<std::string> list = make_list(sizes[(round / 3) % 6], prefix);
        const size_t nw = list.size();
        // the list packed at its exact size
        std::vector<uint64_t> woff(nw + 1, 0);
        for (size_t i = 0; i < nw; ++i) woff[i + 1] = woff[i] + list[i].size();
        std::vector<uint8_t> packed((size_t)woff[nw]);
        for (size_t i = 0; i < nw; ++i) if (!list[i].empty()) std::memcpy(packed.data() + woff[i], list[i].data(), list[i].size());
        // part 1: the tables and the way back through them
        {
            kgpu::VocabTables t;
            std::string err;
            REQUIRE(kgpu::build_vocab_table(nullptr, 0, 0, nullptr, nullptr, nullptr, packed.data(), woff.data(), nw, 0, t, err) == KGPU_OK);
            std::vector<uint32_t> entry;
            kgpu::build_decode_entries(t, nw, entry);
            REQUIRE(entry.size() == nw);
            for (size_t i = 0; i < nw; ++i) {
                const size_t at = (size_t)entry[i] * 8;
                REQUIRE(at + kgpu::COUNT_ENTRY_HEAD + 8 <= t.arena.size());   // the device's one 8-byte load of the head stays inside the arena
                uint32_t len;
                std::memcpy(&len, t.arena.data() + at, 4);
                REQUIRE(len == list[i].size() && at + kgpu::COUNT_ENTRY_HEAD + len <= t.arena.size());
                REQUIRE(len == 0 || std::memcmp(t.arena.data() + at + kgpu::COUNT_ENTRY_HEAD, list[i].data(), len) == 0);
                REQUIRE(kgpu::decode_head(t.arena.data() + at + kgpu::COUNT_ENTRY_HEAD, len) == kgpu::decode_head((const uint8_t *)list[i].data(), len));
            }
            ++tables;
        }
        // part 2: kgpu_decode_host
        for (int rep = 0; rep < 18; ++rep) {
            const std::string &sep = seps[rnd() % 4];
            kgpu_decode_opts o{};
            o.size = (uint32_t)sizeof o;
            o.sep_len = (uint32_t)sep.size();
            std::memcpy(o.sep, sep.data(), sep.size());
            const int32_t odd[] = {-1, (int32_t)nw, INT32_MIN, INT32_MAX};
            const uint32_t skips[] = {0, 1, 8};
            o.n_skip = skips[rnd() % 3];
            for (uint32_t i = 0; i < o.n_skip; ++i) o.skip_ids[i] = rnd() % 2 ? odd[rnd() % 4] : (int32_t)(rnd() % nw);
            const auto one_id = [&]() -> int32_t { const uint32_t r = rnd() % 10; return r == 0 ? odd[rnd() % 4] : (r == 1 && o.n_skip) ? o.skip_ids[rnd() % o.n_skip] : (int32_t)(rnd() % nw); };
            const uint64_t ns[] = {0, 1, 5, 9};
            const uint64_t n = ns[rnd() % 4];
            const bool ragged = rnd() % 2;
            const uint64_t widths[] = {1, 2, 7, 64, 65};
            const uint64_t width = ragged ? 0 : widths[rnd() % 5];
            std::vector<uint64_t> off;
            if (ragged) {
                const uint64_t lens[] = {0, 0, 1, 3, 63, 64, 65, 130};
                off.push_back(rnd() % 3);
                for (uint64_t s = 0; s < n; ++s) off.push_back(off.back() + lens[rnd() % 8]);
            }
            std::vector<int32_t> ids((size_t)(ragged ? off[n] : n * width));   // exactly what the offsets reach
            for (int32_t &id : ids) id = one_id();
            // the naive restatement
            std::vector<std::string> want(n);
            std::vector<uint8_t> want_status(n, 0);
            for (uint64_t s = 0; s < n; ++s) {
                const uint64_t k0 = ragged ? off[s] : s * width, k1 = ragged ? off[s + 1] : (s + 1) * width;
                uint64_t kept = 0;
                for (uint64_t k = k0; k < k1; ++k) {
                    const int32_t id = ids[k];
                    if (skipped(o, id)) continue;
                    if (id < 0 || (uint64_t)id >= nw) { want_status[s] = 1; continue; }
                    const std::string &w = list[(size_t)id];
                    if (kept == 0) want[s] += w;
                    else if (!prefix.empty() && w.compare(0, prefix.size(), prefix) == 0) want[s] += w.substr(prefix.size());
                    else want[s] += sep + w;
                    ++kept;
                }
            }
            uint64_t total = 0;
            for (const std::string &w : want) total += w.size();
            const auto call = [&](uint8_t *text, uint64_t cap, uint64_t *toff, uint8_t *st, uint64_t *got) {
                return kgpu_decode_host(packed.data(), woff.data(), nw, (const uint8_t *)prefix.data(), (uint32_t)prefix.size(), ids.empty() ? nullptr : ids.data(),
                                        ragged ? off.data() : nullptr, n, width, rep % 6 == 0 && sep == " " && o.n_skip == 0 ? nullptr : &o, text, cap, toff, st, got);
            };
            std::vector<uint64_t> toff(n + 1);
            std::vector<uint8_t> st(n);
            uint64_t got = 0;
            if (total) {   // one byte short: the size, and no store
                std::vector<uint8_t> x((size_t)total - 1, 0x5A);
                REQUIRE(call(x.data(), total - 1, toff.data(), st.data(), &got) == KGPU_ERR_CAPACITY && got == total);
                for (uint8_t b : x) REQUIRE(b == 0x5A);
            }
            std::vector<uint8_t> text((size_t)total);
            REQUIRE(call(text.data(), total, toff.data(), st.data(), &got) == KGPU_OK && got == total && toff[0] == 0 && toff[n] == total);
            for (uint64_t s = 0; s < n; ++s) {
                REQUIRE(toff[s + 1] - toff[s] == want[s].size() && st[s] == want_status[s]);
                REQUIRE(want[s].empty() || std::memcmp(text.data() + toff[s], want[s].data(), want[s].size()) == 0);
            }
            ++calls;
        }
    }
    std::printf("decode sanitized ok %llu %llu\n", (unsigned long long)calls, (unsigned long long)tables);
    return 0;
}
