// tests/c_abi/normalize_main.cpp -- kgpu_normalize_table.cpp alone, under the sanitizers (tests/test_normalize_cpu.py builds both with plain g++): the host
// normaliser over a file of cases, each with capacities of 0, exact - 1 and exact.  The file: per case one line `<form> <status> <input hex or -> <expected hex or ->`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_internal.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (declared by the header; the calls below check the return codes)
}

static std::vector<uint8_t> unhex(const char *s) {
    std::vector<uint8_t> out;
    if (std::strcmp(s, "-") == 0) return out;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        const char b[3] = {s[i], s[i + 1], 0};
        out.push_back((uint8_t)std::strtoul(b, nullptr, 16));
    }
    return out;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::printf("line %d (case %d): %s\n", __LINE__, n_cases, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv) {
    int n_cases = 0;
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    static char in_hex[1 << 16], out_hex[1 << 18];
    int form, status;
    while (std::fscanf(f, "%d %d %65535s %262143s", &form, &status, in_hex, out_hex) == 4) {
        ++n_cases;
        const std::vector<uint8_t> in = unhex(in_hex), want = unhex(out_hex);
        uint64_t need = 123;
        uint8_t st = 99;
        // capacity 0 with a null buffer: the exact size, nothing written
        int rc = kgpu_normalize_host(form, in.data(), in.size(), nullptr, 0, &need, &st);
        REQUIRE(need == want.size() && st == status);
        REQUIRE(rc == (want.empty() ? KGPU_OK : KGPU_ERR_CAPACITY));
        // exact - 1, in a heap block of exactly that size: one byte more written is a sanitizer report
        if (!want.empty()) {
            uint8_t *small = (uint8_t *)std::malloc(want.size() - 1 ? want.size() - 1 : 1);
            if (want.size() > 1) std::memset(small, 0x5A, want.size() - 1);
            rc = kgpu_normalize_host(form, in.data(), in.size(), small, want.size() - 1, &need, &st);
            REQUIRE(rc == KGPU_ERR_CAPACITY && need == want.size());
            for (size_t i = 0; i + 1 < want.size(); ++i) REQUIRE(small[i] == 0x5A);
            std::free(small);
        }
        // exact
        uint8_t *out = (uint8_t *)std::malloc(want.size() ? want.size() : 1);
        rc = kgpu_normalize_host(form, in.data(), in.size(), out, want.size(), &need, &st);
        REQUIRE(rc == KGPU_OK && need == want.size() && st == status);
        REQUIRE(want.empty() || std::memcmp(out, want.data(), want.size()) == 0);
        std::free(out);
    }
    std::fclose(f);
    uint64_t need = 0;
    const uint8_t a = 'a';
    uint8_t o = 0;
    if (kgpu_normalize_host(0, &a, 1, &o, 1, &need, nullptr) != KGPU_ERR_INVALID_ARG || kgpu_normalize_host(3, &a, 1, &o, 1, &need, nullptr) != KGPU_ERR_INVALID_ARG ||
        kgpu_normalize_host(1, nullptr, 1, &o, 1, &need, nullptr) != KGPU_ERR_INVALID_ARG || kgpu_normalize_host(1, &a, 1, nullptr, 1, &need, nullptr) != KGPU_ERR_INVALID_ARG ||
        kgpu_normalize_host(1, &a, 1, &o, 1, nullptr, nullptr) != KGPU_ERR_INVALID_ARG) {
        std::printf("argument errors\n");
        return 1;
    }
    if (!kgpu_normalize_unicode_version()[0]) return 1;
    std::printf("normalize ok: %d cases\n", n_cases);
    return n_cases ? 0 : 1;
}
