// kanpyo_amd/csrc/kgpu_decode_core.h -- the rule of the text from ids (include/kanpyo_gpu.h, "text from ids"), written once for the host
// (kgpu_decode_host.cpp: kgpu_decode_host) and for the device (kgpu_decode.hip): the same statements decide both.  Plain C++ without a HIP include.
// Two steps per element, each O(1):
//   decode_class   rule 1: is the id skipped, out of the list's range (the status bit), or a KEPT element
//   decode_piece   rule 2: what a kept element contributes -- `sep` separator bytes, then the word's bytes [skip, skip + len)
// A piece may be EMPTY (the empty word as kept element 0, a word equal to the prefix, the empty word behind an empty separator): such an element
// still counts as a kept element -- the one behind it is not element 0 -- but has no byte, so the write pass leaves it out of its pieces.
// Words are looked at through their length and their first eight bytes alone (`head`, byte i in bits 8 i ..; bytes behind the word's end: anything).
#pragma once
#include <cstdint>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_normalize_core.h"   // KGPU_NORM_HD

namespace kgpu {

struct DecodeRule {               // kgpu_decode_opts, the prefix and the list's size as the kernels take them
    uint32_t n_words;
    uint32_t sep_len, prefix_len, n_skip;
    uint64_t sep, prefix;         // byte i in bits 8 i ..
    int32_t skip[KGPU_DECODE_MAX_SKIP];
};

struct DecodeClass { bool kept, bad; };
struct DecodePiece {
    uint32_t sep, skip, len;      // the separator's bytes in front, then the word without its first `skip` bytes: `len` of them
    KGPU_NORM_HD uint64_t bytes() const { return (uint64_t)sep + len; }
};

KGPU_NORM_HD uint64_t decode_low_bytes(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8 * n)) - 1; }   // a mask of the first n bytes of a head

// rule 1
KGPU_NORM_HD DecodeClass decode_class(const DecodeRule &r, int32_t id) {
    bool skipped = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < KGPU_DECODE_MAX_SKIP; ++i) skipped = skipped || (i < r.n_skip && r.skip[i] == id);
    if (skipped) return DecodeClass{false, false};
    if (id < 0 || (uint32_t)id >= r.n_words) return DecodeClass{false, true};
    return DecodeClass{true, false};
}

// rule 2: first -- no kept element stands in front of this one in its sequence
KGPU_NORM_HD DecodePiece decode_piece(const DecodeRule &r, bool first, uint32_t word_len, uint64_t head) {
    if (first) return DecodePiece{0, 0, word_len};
    if (r.prefix_len && word_len >= r.prefix_len && ((head ^ r.prefix) & decode_low_bytes(r.prefix_len)) == 0)
        return DecodePiece{0, r.prefix_len, word_len - r.prefix_len};   // the prefix goes, once
    return DecodePiece{r.sep_len, 0, word_len};
}

// The first eight bytes of a word (fewer when it is shorter) as decode_piece takes them.
inline uint64_t decode_head(const uint8_t *p, uint64_t len) {
    uint64_t h = 0;
    for (uint32_t i = 0; i < 8 && i < len; ++i) h |= (uint64_t)p[i] << (8 * i);
    return h;
}

// The options' part of the argument check -> what is wrong, or null
inline const char *decode_opts_error(const kgpu_decode_opts *o, uint32_t prefix_len) {
    if (prefix_len > 8) return "prefix_len is above 8";
    if (!o) return nullptr;
    if (o->size < sizeof(kgpu_decode_opts)) return "opts.size is smaller than the struct";
    if (o->flags) return "unknown flags";
    if (o->sep_len > 8) return "sep_len is above 8";
    if (o->n_skip > KGPU_DECODE_MAX_SKIP) return "n_skip is above KGPU_DECODE_MAX_SKIP";
    return nullptr;
}
// (o null: one space, no skip list)
inline DecodeRule decode_rule(const kgpu_decode_opts *o, const uint8_t *prefix, uint32_t prefix_len, uint64_t n_words) {
    DecodeRule r{(uint32_t)n_words, 1, prefix_len, 0, (uint64_t)' ', prefix_len ? decode_head(prefix, prefix_len) : 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    if (o) {
        r.sep_len = o->sep_len; r.sep = decode_head(o->sep, o->sep_len);
        r.n_skip = o->n_skip;
        for (uint32_t i = 0; i < o->n_skip; ++i) r.skip[i] = o->skip_ids[i];
    }
    return r;
}

}  // namespace kgpu
