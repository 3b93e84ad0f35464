// tests/c_abi/align_main.cpp -- kgpu_normalize_table.cpp alone, under the sanitizers (tests/test_align_cpu.py builds both with plain g++): the host side of the
// source alignment over a file of cases.  Per case one line:
//   N <form> <status> <input hex or -> <expected hex or -> <n edits> <8 numbers per edit>        kgpu_normalize_host_aligned, every capacity protocol case
//   S <n edits> <8 numbers per edit> <n tokens> <4 numbers per token> <4 numbers per span>      kgpu_source_spans_host over one sentence
// Every buffer is a heap block of exactly the size the call is told: one record more written is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../kanpyo_amd/csrc/kgpu_internal.h"

namespace kgpu {
void set_error(const char *, ...) {}   // (declared by the header; the calls below check the return codes)
}

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}
static std::vector<kgpu_norm_edit> read_edits(std::istream &in) {
    size_t n = 0;
    in >> n;
    std::vector<kgpu_norm_edit> e(n);
    for (auto &x : e) {
        uint32_t v[8];
        for (auto &w : v) in >> w;
        x = kgpu_norm_edit{v[0], v[1], v[2], v[3], (uint16_t)v[4], (uint16_t)v[5], (uint16_t)v[6], (uint16_t)v[7]};
    }
    return e;
}
template <class T> static T *exact(size_t n, int fill) {   // a block of exactly n records (one byte when n is 0: never to be touched)
    T *p = (T *)std::malloc(n ? n * sizeof(T) : 1);
    std::memset(p, fill, n ? n * sizeof(T) : 1);
    return p;
}
template <class T> static bool untouched(const T *p, size_t n, int fill) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n * sizeof(T); ++i)
        if (b[i] != (uint8_t)fill) return false;
    return true;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::printf("line %d (case %d): %s\n", __LINE__, n_cases, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv) {
    int n_cases = 0;
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string kind;
    while (f >> kind) {
        ++n_cases;
        if (kind == "N") {
            int form, status;
            std::string in_hex, out_hex;
            f >> form >> status >> in_hex >> out_hex;
            const std::vector<uint8_t> in = unhex(in_hex), want = unhex(out_hex);
            const std::vector<kgpu_norm_edit> we = read_edits(f);
            const size_t nb = want.size(), ne = we.size();
            // both exact: written, and equal
            {
                uint8_t *out = exact<uint8_t>(nb, 0xEE);
                kgpu_norm_edit *ed = exact<kgpu_norm_edit>(ne, 0xEE);
                uint64_t need = 123, nedits = 456;
                uint8_t st = 99;
                const int rc = kgpu_normalize_host_aligned(form, in.data(), in.size(), out, nb, &need, &st, ed, ne, &nedits);
                REQUIRE(rc == KGPU_OK && need == nb && nedits == ne && st == status);
                REQUIRE(nb == 0 || std::memcmp(out, want.data(), nb) == 0);
                REQUIRE(ne == 0 || std::memcmp(ed, we.data(), ne * sizeof(kgpu_norm_edit)) == 0);
                std::free(out); std::free(ed);
            }
            // text one short, edits one short, both: the two exact sizes, nothing written to either
            for (int which = 1; which <= 3; ++which) {
                const bool short_text = which & 1, short_edits = which & 2;
                if ((short_text && nb == 0) || (short_edits && ne == 0)) continue;
                const size_t cb = nb - (short_text ? 1 : 0), ce = ne - (short_edits ? 1 : 0);
                uint8_t *out = exact<uint8_t>(cb, 0xEE);
                kgpu_norm_edit *ed = exact<kgpu_norm_edit>(ce, 0xEE);
                uint64_t need = 123, nedits = 456;
                const int rc = kgpu_normalize_host_aligned(form, in.data(), in.size(), out, cb, &need, nullptr, ed, ce, &nedits);
                REQUIRE(rc == KGPU_ERR_CAPACITY && need == nb && nedits == ne);
                REQUIRE(untouched(out, cb, 0xEE) && untouched(ed, ce, 0xEE));
                std::free(out); std::free(ed);
            }
            // no buffers at all: the sizes
            uint64_t need = 1, nedits = 1;
            const int rc = kgpu_normalize_host_aligned(form, in.data(), in.size(), nullptr, 0, &need, nullptr, nullptr, 0, &nedits);
            REQUIRE(need == nb && nedits == ne && rc == ((nb || ne) ? KGPU_ERR_CAPACITY : KGPU_OK));
        } else if (kind == "S") {
            const std::vector<kgpu_norm_edit> e = read_edits(f);
            size_t nt = 0;
            f >> nt;
            std::vector<kgpu_token> t(nt);
            std::vector<kgpu_span> want(nt);
            for (auto &x : t) { f >> x.position >> x.byte_len >> x.start >> x.end; x.id = 1; x.cls = x.byte_len ? KGPU_CLASS_KNOWN : KGPU_CLASS_DUMMY; }
            for (auto &x : want) f >> x.position >> x.byte_len >> x.start >> x.end;
            // the sentence between two empty ones, and the records behind three that belong to nobody: tok_offsets[0] is not 0
            kgpu_token *tok = exact<kgpu_token>(nt + 3, 0x11);
            if (nt) std::memcpy(tok + 3, t.data(), nt * sizeof(kgpu_token));
            kgpu_norm_edit *ed = exact<kgpu_norm_edit>(e.size(), 0);
            if (!e.empty()) std::memcpy(ed, e.data(), e.size() * sizeof(kgpu_norm_edit));
            kgpu_span *sp = exact<kgpu_span>(nt, 0xEE);
            const uint64_t toff[4] = {3, 3, 3 + nt, 3 + nt}, eoff[4] = {0, 0, e.size(), e.size()};
            kgpu_source_spans_host(tok, toff, 3, ed, eoff, sp);
            REQUIRE(nt == 0 || std::memcmp(sp, want.data(), nt * sizeof(kgpu_span)) == 0);
            std::free(tok); std::free(ed); std::free(sp);
        } else {
            std::printf("unknown record %s\n", kind.c_str());
            return 2;
        }
        if (!f) { std::printf("case %d: truncated\n", n_cases); return 2; }
    }
    uint64_t need = 0, nedits = 0;
    const uint8_t a = 'a';
    uint8_t o = 0;
    kgpu_norm_edit e1;
    if (kgpu_normalize_host_aligned(0, &a, 1, &o, 1, &need, nullptr, &e1, 1, &nedits) != KGPU_ERR_INVALID_ARG ||
        kgpu_normalize_host_aligned(1, &a, 1, &o, 1, &need, nullptr, nullptr, 1, &nedits) != KGPU_ERR_INVALID_ARG ||
        kgpu_normalize_host_aligned(1, &a, 1, &o, 1, &need, nullptr, &e1, 1, nullptr) != KGPU_ERR_INVALID_ARG ||
        kgpu_normalize_host_aligned(1, &a, 1, &o, 1, nullptr, nullptr, &e1, 1, &nedits) != KGPU_ERR_INVALID_ARG) {
        std::printf("argument errors\n");
        return 1;
    }
    std::printf("align ok: %d cases\n", n_cases);
    return n_cases ? 0 : 1;
}
