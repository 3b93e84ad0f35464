// kanpyo_amd/csrc/kgpu_decode_host.cpp -- kgpu_decode_host: the text from ids (include/kanpyo_gpu.h, "text from ids") on the host, the definition of what
// kgpu_decode.hip writes.  HIP-free, compiles alone (with a set_error of the caller's: tests/c_abi/decode_sanitize.cpp): decode_class and decode_piece
// of kgpu_decode_core.h decide every element here as they do on the device; this file adds the loops and the argument checks, which the device
// forms share (decode_check_args).
#include <cstring>

#include "kgpu_internal.h"

int kgpu::decode_check_args(const char *who, const void *ids, const void *id_offsets, bool host_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *o,
                            uint32_t prefix_len, const void *text, uint64_t text_capacity, const void *text_offsets, const void *status) {
    if (const char *why = decode_opts_error(o, prefix_len)) { set_error("%s: %s", who, why); return KGPU_ERR_INVALID_ARG; }
    if ((id_offsets != nullptr) == (width != 0)) { set_error("%s: id_offsets with width 0 (ragged), or no id_offsets and a width of 1 or more (padded)", who); return KGPU_ERR_INVALID_ARG; }
    if (!text_offsets || (n && !status) || (text_capacity && !text)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (width && n > (~0ull >> 3) / width) { set_error("%s: n x width does not fit an address", who); return KGPU_ERR_INVALID_ARG; }
    uint64_t n_ids = n * width;
    if (host_offsets && id_offsets) {
        const uint64_t *off = (const uint64_t *)id_offsets;
        for (uint64_t s = 0; s < n; ++s)
            if (off[s + 1] < off[s]) { set_error("%s: id offsets run backwards at sequence %llu", who, (unsigned long long)s); return KGPU_ERR_INVALID_ARG; }
        n_ids = off[n] - off[0];
    }
    // (ragged offsets in device memory: the count is theirs to say, and empty sequences read no id)
    if (n_ids && !ids) { set_error("%s: null ids", who); return KGPU_ERR_INVALID_ARG; }
    if ((uintptr_t)ids & 3u) { set_error("%s: ids is not 4-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    if (((uintptr_t)id_offsets | (uintptr_t)text_offsets) & 7u) { set_error("%s: an offsets array is not 8-byte aligned", who); return KGPU_ERR_INVALID_ARG; }
    return KGPU_OK;
}

extern "C" int kgpu_decode_host(const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const uint8_t *prefix, uint32_t prefix_len,
                                const int32_t *ids, const uint64_t *id_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *opts,
                                uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes) {
    const char *who = "kgpu_decode_host";
    using namespace kgpu;
    if (n_bytes) *n_bytes = 0;
    if (int rc = decode_check_args(who, ids, id_offsets, true, n, width, opts, prefix_len, text, text_capacity, text_offsets, status)) return rc;
    if ((n_words && !word_offsets) || (prefix_len && !prefix) || n_words > 0x7FFFFFFFull) { set_error("%s: null argument, or more than 2^31 - 1 words", who); return KGPU_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n_words; ++i)
        if (word_offsets[i + 1] < word_offsets[i] || word_offsets[i + 1] - word_offsets[i] >= (1ull << 30)) {
            set_error("%s: word offsets run backwards at %llu, or the word has 2^30 bytes or more", who, (unsigned long long)i);
            return KGPU_ERR_INVALID_ARG;
        }
    if (n_words && word_offsets[n_words] != word_offsets[0] && !words) { set_error("%s: word offsets without words", who); return KGPU_ERR_INVALID_ARG; }
    const DecodeRule r = decode_rule(opts, prefix, prefix_len, n_words);
    uint8_t sep[8];
    for (uint32_t i = 0; i < 8; ++i) sep[i] = (uint8_t)(r.sep >> (8 * i));
    // The walk of one sequence, for both passes: emit(piece, the word's first byte) for every kept element, in order -> the status byte.
    const auto walk = [&](uint64_t s, auto &&emit) {
        const uint64_t k0 = id_offsets ? id_offsets[s] : s * width, k1 = id_offsets ? id_offsets[s + 1] : (s + 1) * width;
        bool seen = false, bad = false;
        for (uint64_t k = k0; k < k1; ++k) {
            const DecodeClass c = decode_class(r, ids[k]);
            bad = bad || c.bad;
            if (!c.kept) continue;
            const uint8_t *w = words + word_offsets[ids[k]];
            const uint64_t len = word_offsets[ids[k] + 1] - word_offsets[ids[k]];
            emit(decode_piece(r, !seen, (uint32_t)len, len ? decode_head(w, len) : 0), w);
            seen = true;
        }
        return (uint8_t)(bad ? KGPU_DECODE_BAD_ID : KGPU_DECODE_OK);
    };
    // the length pass: the lines' bytes, the status bytes, the scan
    uint64_t total = 0;
    for (uint64_t s = 0; s < n; ++s) {
        text_offsets[s] = total;
        status[s] = walk(s, [&](const DecodePiece &p, const uint8_t *) { total += p.bytes(); });
    }
    text_offsets[n] = total;
    if (n_bytes) *n_bytes = total;
    if (total > text_capacity) {
        set_error("%s: text buffer too small: need %llu, capacity %llu", who, (unsigned long long)total, (unsigned long long)text_capacity);
        return KGPU_ERR_CAPACITY;
    }
    // the write pass
    for (uint64_t s = 0; s < n; ++s) {
        uint8_t *out = text + text_offsets[s];
        walk(s, [&](const DecodePiece &p, const uint8_t *w) {
            if (p.sep) std::memcpy(out, sep, p.sep);
            if (p.len) std::memcpy(out + p.sep, w + p.skip, p.len);
            out += p.bytes();
        });
    }
    return KGPU_OK;
}
