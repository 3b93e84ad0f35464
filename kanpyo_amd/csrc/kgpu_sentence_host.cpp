// kanpyo_amd/csrc/kgpu_sentence_host.cpp -- kgpu_split_sentences_host: lines cut into sentences (include/kanpyo_gpu.h, "sentences") on the host, the
// definition of what kgpu_sentence.hip writes.  HIP-free, compiles alone (with a set_error of the caller's): the classes and the two depth walks of
// kgpu_sentence_core.h decide every boundary here as they do on the device; this file adds the loops, the options' check and the argument checks.
#include <vector>

#include "kgpu_internal.h"

namespace {

using namespace kgpu;

bool is_white_space(uint32_t cp) {
    return (cp >= 9 && cp <= 13) || cp == 0x20 || cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) || cp == 0x2028 || cp == 0x2029 ||
           cp == 0x202F || cp == 0x205F || cp == 0x3000;
}

// (cp is a scalar value: the window of its encoding)
uint32_t encode_window(uint32_t cp, uint32_t &mask) {
    if (cp < 0x80) { mask = 0xFFu; return cp; }
    if (cp < 0x800) { mask = 0xFFFFu; return (0xC0u | (cp >> 6)) | ((0x80u | (cp & 0x3Fu)) << 8); }
    if (cp < 0x10000) { mask = 0xFFFFFFu; return (0xE0u | (cp >> 12)) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 8) | ((0x80u | (cp & 0x3Fu)) << 16); }
    mask = 0xFFFFFFFFu;
    return (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 0x3Fu)) << 8) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 16) | ((0x80u | (cp & 0x3Fu)) << 24);
}

inline uint32_t window_at(const uint8_t *s, uint64_t i, uint64_t len) {
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4 && i + k < len; ++k) w |= (uint32_t)s[i + k] << (8 * k);
    return w;
}

// The sentences of a line behind its first, in order: where the sentence in front ends (the boundary), where this one starts.
struct Cut { uint64_t end, start; };
void line_starts(const SentRule &rule, const uint8_t *s, uint64_t len, std::vector<uint8_t> &tl, std::vector<uint8_t> &zero, std::vector<Cut> &starts) {
    starts.clear();
    tl.assign((size_t)len + 1, 0); zero.assign((size_t)len + 1, 0);
    bool any = false;
    for (uint64_t i = 0; i < len; ++i) any |= (tl[i] = (uint8_t)sent_term_len(rule, window_at(s, i, len))) != 0;
    if (!any) return;
    const auto delta = [&](uint64_t i) { return rule.no_brackets ? 0 : sent_bracket(window_at(s, i, len)); };
    int64_t v = 0;
    for (uint64_t j = 0; j < len; ++j) { v = sent_apply(sent_fwd_step<int64_t>(delta(j), j == 0), v); zero[j] = v == 0; }
    int64_t u = 0;
    for (uint64_t j = len; j-- > 0;) { u = sent_apply(sent_bwd_step<int64_t>(j + 1 < len ? delta(j + 1) : 0, j + 1 == len), u); zero[j] |= u == 0; }
    for (uint64_t i = 0; i < len;) {
        if (!tl[i]) { ++i; continue; }
        const uint64_t e = i + tl[i];
        if (!tl[e] && zero[i]) {   // the run ends here, outside every matched pair: a boundary
            uint64_t p = e;
            for (uint32_t l; p < len && (l = sent_space_len(window_at(s, p, len))) != 0;) p += l;
            if (p < len) starts.push_back(Cut{e, p});
        }
        i = e;
    }
}

}  // namespace

int kgpu::sent_rule_from_opts(const char *who, const kgpu_sentence_opts *o, SentRule &rule) {
    static const uint32_t DEFAULTS[6] = {0x3002, 0xFF61, 0xFF01, 0xFF1F, '!', '?'};
    rule = SentRule{};
    const uint32_t *cps = DEFAULTS;
    uint32_t n = 6;
    if (o) {
        if ((o->flags & ~KGPU_SENTENCES_NO_BRACKETS) || o->reserved[0] || o->reserved[1]) { set_error("%s: an unknown flag or a reserved word is set", who); return KGPU_ERR_INVALID_ARG; }
        if (o->n_terminators > SENT_MAX_TERMINATORS) { set_error("%s: %u terminators, at most %u", who, o->n_terminators, SENT_MAX_TERMINATORS); return KGPU_ERR_INVALID_ARG; }
        rule.no_brackets = o->flags & KGPU_SENTENCES_NO_BRACKETS;
        if (o->n_terminators) { cps = o->terminators; n = o->n_terminators; }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t cp = cps[i];
        uint32_t mask = 0;
        const uint32_t pat = cp < 0x110000 ? encode_window(cp, mask) : 0;
        if (cp < 0x21 || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF) || is_white_space(cp) || sent_bracket(pat) != 0) {
            set_error("%s: terminator U+%04X is below U+0021, no scalar value, White_Space or a bracket", who, cp);
            return KGPU_ERR_INVALID_ARG;
        }
        rule.pat[i] = pat; rule.mask[i] = mask;
    }
    for (uint32_t i = n; i < SENT_MAX_TERMINATORS; ++i) { rule.pat[i] = ~0u; rule.mask[i] = 0; }
    rule.n_term = n;
    return KGPU_OK;
}

extern "C" int kgpu_split_sentences_host(const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_sentence_opts *opts, uint8_t *out,
                                         uint64_t *out_offsets, kgpu_sentence *sents, uint64_t sent_capacity, uint64_t *n_sentences) {
    const char *who = "kgpu_split_sentences_host";
    using namespace kgpu;
    if (n_sentences) *n_sentences = 0;
    if (!offsets || !n_sentences || !out_offsets || (sent_capacity && !sents)) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    SentRule rule;
    if (int rc = sent_rule_from_opts(who, opts, rule)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) { set_error("%s: offsets run backwards at line %llu", who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
    const uint64_t total = offsets[n] - offsets[0];
    if (total >= (1ull << 32)) { set_error("%s: 4 GiB of text or more; split the batch", who); return KGPU_ERR_INVALID_ARG; }
    if (total && !utf8) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    // first the count, then the stores: nothing is written when the sentences do not fit
    std::vector<uint8_t> tl, zero;
    std::vector<Cut> starts;
    uint64_t S = 0;
    for (uint64_t i = 0; i < n; ++i) {
        line_starts(rule, total ? utf8 + offsets[i] : nullptr, offsets[i + 1] - offsets[i], tl, zero, starts);
        S += 1 + starts.size();
    }
    *n_sentences = S;
    if (S > sent_capacity) { set_error("%s: %llu sentences, capacity %llu", who, (unsigned long long)S, (unsigned long long)sent_capacity); return KGPU_ERR_CAPACITY; }
    if (total && !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    uint64_t k = 0, at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t *s = total ? utf8 + offsets[i] : nullptr;
        const uint64_t len = offsets[i + 1] - offsets[i];
        line_starts(rule, s, len, tl, zero, starts);
        starts.push_back(Cut{len, len});   // (the end of the last sentence)
        uint64_t b = 0, chars = 0, counted = 0;
        for (const Cut &c : starts) {
            for (; counted < b; ++counted) chars += (s[counted] & 0xC0u) != 0x80u;
            out_offsets[k] = at;
            sents[k] = kgpu_sentence{i, (uint32_t)b, (uint32_t)chars};
            for (uint64_t x = b; x < c.end; ++x) out[at++] = s[x];
            ++k;
            b = c.start;
        }
    }
    out_offsets[k] = at;
    return KGPU_OK;
}
