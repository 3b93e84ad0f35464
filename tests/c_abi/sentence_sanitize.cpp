// tests/c_abi/sentence_sanitize.cpp -- kgpu_split_sentences_host (kanpyo_amd/csrc/kgpu_sentence_host.cpp, compiled with this file alone) over seeded lines
// dense in every class of the rule, in buffers of exactly the size needed: what the sanitizers watch.  A stand-alone program: nothing is loaded into Python.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kanpyo_gpu.h"

namespace kgpu {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    va_end(ap);
    (void)fmt;
}
}  // namespace kgpu

int main() {
    const char *alphabet[] = {"。", "｡", "！", "？", "!", "?", "「", "」", "（", "）", "(", ")", "[", "]", "【", "】", " ", "\t", "　", "\xc2\xa0", "\xe2\x80\x83",
                              "あ", "a", ".", "\xe3", "\x80", "\xef\xbc", "\xe2\x80", "\xc2"};
    const size_t A = sizeof(alphabet) / sizeof(alphabet[0]);
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const auto next = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    uint64_t sentences = 0;
    for (int round = 0; round < 400; ++round) {
        std::string text;
        std::vector<uint64_t> offsets{0};
        const uint64_t n = next() % 6;
        for (uint64_t i = 0; i < n; ++i) {
            for (uint64_t k = next() % 40; k > 0; --k) text += alphabet[next() % A];
            offsets.push_back(text.size());
        }
        kgpu_sentence_opts o;
        std::memset(&o, 0, sizeof o);
        o.flags = round % 3 == 0 ? KGPU_SENTENCES_NO_BRACKETS : 0u;
        if (round % 5 == 0) { o.n_terminators = 2; o.terminators[0] = '.'; o.terminators[1] = 0x3042; }
        uint64_t S = 0, probe = 0;
        std::vector<uint8_t> in(text.begin(), text.end());
        if (kgpu_split_sentences_host(in.data(), offsets.data(), n, &o, nullptr, &probe, nullptr, 0, &S) != (n ? KGPU_ERR_CAPACITY : KGPU_OK)) return 1;
        std::vector<uint8_t> out(text.size());
        std::vector<uint64_t> ooff(S + 1);
        std::vector<kgpu_sentence> recs(S);
        uint64_t S2 = 0;
        if (kgpu_split_sentences_host(in.data(), offsets.data(), n, &o, out.data(), ooff.data(), recs.data(), S, &S2) != KGPU_OK || S2 != S) return 2;
        if (S < n || ooff[S] > text.size()) return 3;
        sentences += S;
    }
    std::printf("sentence sanitize ok: %llu sentences\n", (unsigned long long)sentences);
    return 0;
}
