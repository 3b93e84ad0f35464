// kanpyo_amd/csrc/kgpu_sentence_core.h -- the sentence rule (include/kanpyo_gpu.h, "sentences"), written once for the host (kgpu_sentence_host.cpp:
// kgpu_split_sentences_host) and for the device (kgpu_sentence.hip): the same statements decide a byte's class and a terminator's enclosing depth on
// both, so that the device result IS the host result.  Plain C++; HIP-free unless a HIP compiler reads it.
//
// A class is looked up in a WINDOW: the four bytes at a position of a line, little-endian, zero where the line has ended.  No pattern holds a zero byte,
// so an encoding the line's end cuts short matches nothing.
//
// The enclosing depth of byte j, eff(j) = r(j) - max(P(j), S(j)) (r: openers minus closers over 0..j; P: min(0, min r over 0..j); S: min r over j..end), is
// zero exactly when v(j) == 0 or u(j) == 0, where
//     v(j) = P(j) - r(j) = min(0, v(j - 1) - d(j)),  v(-1) = 0          (d: +1 at an opener's first byte, -1 at a closer's, else 0)
//     u(j) = S(j) - r(j) = min(0, u(j + 1) + d(j + 1)),  u(last) = 0
// Both are compositions of x -> min(a, x + b): SentFn, closed under composition, with a constant function where a line starts -- what the kernels scan.
#pragma once
#include <stdint.h>

#include "kgpu_normalize_core.h"   // KGPU_NORM_HD

namespace kgpu {

constexpr uint32_t SENT_MAX_TERMINATORS = 16;
// The terminators as windows: pat[i] is terminator i's UTF-8 encoding, little-endian; mask[i] covers its bytes.  An entry at or behind n_term has
// mask 0 and pat ~0 and matches nothing: every lookup walks all sixteen, unrolled, with no load inside the loop.
struct SentRule { uint32_t n_term, no_brackets; uint32_t pat[SENT_MAX_TERMINATORS], mask[SENT_MAX_TERMINATORS]; };

KGPU_NORM_HD uint32_t sent_mask_len(uint32_t mask) { return mask == 0xFFu ? 1u : mask == 0xFFFFu ? 2u : mask == 0xFFFFFFu ? 3u : 4u; }

// The length of the terminator whose encoding starts the window; 0: none does.
KGPU_NORM_HD uint32_t sent_term_len(const SentRule &r, uint32_t w) {
    uint32_t len = 0;
#ifdef __clang__   // (a pragma gcc does not know)
#pragma unroll
#endif
    for (uint32_t i = 0; i < SENT_MAX_TERMINATORS; ++i)
        if ((w & r.mask[i]) == r.pat[i]) len = sent_mask_len(r.mask[i]);
    return len;
}

// The length of the White_Space encoding that starts the window (the 25 code points of kgpu_split_lines); 0: none does.
KGPU_NORM_HD uint32_t sent_space_len(uint32_t w) {
    const uint32_t b0 = w & 0xFFu, t2 = w & 0xFFFFu, t = w & 0xFFFFFFu;
    if (b0 - 9u <= 4u || b0 == 0x20u) return 1;
    if (t2 == 0x85C2u || t2 == 0xA0C2u) return 2;   // U+0085, U+00A0
    const uint32_t d = t - 0x8080E2u;               // E2 80 80 .. E2 80 8A: U+2000-200A
    if (((d & 0xFFFFu) == 0 && d <= 0x0A0000u) || t == 0x809AE1u /* U+1680 */ || t == 0xA880E2u || t == 0xA980E2u /* U+2028, 2029 */ ||
        t == 0xAF80E2u /* U+202F */ || t == 0x9F81E2u /* U+205F */ || t == 0x8080E3u /* U+3000 */) return 3;
    return 0;
}

// +1: an opener's encoding starts the window; -1: a closer's; 0: neither.  U+3008-3011 and U+3014-3015 alternate opener, closer; so do U+FF08-FF09 and
// U+FF62-FF63; U+FF3B / FF3D and U+FF5B / FF5D are two apart.
KGPU_NORM_HD int32_t sent_bracket(uint32_t w) {
    const uint32_t b0 = w & 0xFFu, t2 = w & 0xFFFFu, x = ((w >> 16) & 0xFFu) - 0x80u;   // x: the low six bits of a three-byte encoding's code point
    if (b0 == '(' || b0 == '[' || b0 == '{') return 1;
    if (b0 == ')' || b0 == ']' || b0 == '}') return -1;
    if (x > 0x3Fu) return 0;
    if (t2 == 0x80E3u) return ((x >= 0x08u && x <= 0x11u) || x == 0x14u || x == 0x15u) ? ((x & 1u) ? -1 : 1) : 0;   // U+3000 + x
    if (t2 == 0xBCEFu) return (x == 0x08u || x == 0x3Bu) ? 1 : (x == 0x09u || x == 0x3Du) ? -1 : 0;                  // U+FF00 + x
    if (t2 == 0xBDEFu) return (x == 0x1Bu || x == 0x22u) ? 1 : (x == 0x1Du || x == 0x23u) ? -1 : 0;                  // U+FF40 + x
    return 0;
}

// x -> fixed ? a : min(a, x + b), for x <= 0.  {0, 0, 0} maps every such x to itself.
template <class I> struct SentFn { I b, a; uint32_t fixed; };
template <class I> KGPU_NORM_HD SentFn<I> sent_then(const SentFn<I> &f, const SentFn<I> &g) {   // g after f
    if (g.fixed) return g;
    const I fa = f.a + g.b;
    return SentFn<I>{(I)(f.b + g.b), g.a < fa ? g.a : fa, f.fixed};
}
template <class I> KGPU_NORM_HD I sent_apply(const SentFn<I> &f, I x) {
    if (f.fixed) return f.a;
    const I y = x + f.b;
    return f.a < y ? f.a : y;
}
// One byte of the forward walk: v(j) from v(j - 1).  d: the byte's own delta; head: a line starts at it.
template <class I> KGPU_NORM_HD SentFn<I> sent_fwd_step(int32_t d, bool head) {
    return head ? SentFn<I>{0, (I)(d > 0 ? -1 : 0), 1u} : SentFn<I>{(I)-d, 0, 0u};
}
// One byte of the backward walk: u(j) from u(j + 1).  d_next: the delta of byte j + 1; last: the line ends behind byte j.
template <class I> KGPU_NORM_HD SentFn<I> sent_bwd_step(int32_t d_next, bool last) {
    return last ? SentFn<I>{0, 0, 1u} : SentFn<I>{(I)d_next, 0, 0u};
}

}  // namespace kgpu
