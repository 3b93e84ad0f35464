// kanpyo_amd/csrc/kgpu_normalize_core.h -- NFC / NFKC of one segment of a line (include/kanpyo_gpu.h, "text normalisation"), written once for the host
// (kgpu_normalize_table.cpp: kgpu_normalize_host) and for the device (kgpu_normalize.hip): the same statements decide both, so that the device result IS the
// host result.  Plain C++ without a HIP include; under hipcc the functions are __host__ __device__.
//
// The tables (tools/gen_normalize_tables.py derives them, kgpu_normalize_data.inc holds them in a compact form, kgpu_normalize_table.cpp expands that):
//   stage1[cp >> 7] -> block, stage2[block * 128 + (cp & 127)] -> the property word of cp
//       bits 0-7 combining class | bit 8 / 9 NFC boundary before, inert | bit 10 / 11 NFKC boundary before, inert | bit 12 Hangul syllable |
//       bits 13-31 k + 1: dec[2 k] (canonical) / dec[2 k + 1] (compatibility) = offset << 8 | length of the FULL decomposition in pool, length 0: itself
//   pool      code points with their combining class in bits 24-31
//   comp_key  first << 21 | second of the primary composition pairs, ascending; comp_val: the composite (always a starter)
// A buffer entry is a pool entry: code point | combining class << 24.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KGPU_NORM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KGPU_NORM_HD inline
#endif

namespace kgpu {

struct NormTables {
    const uint16_t *stage1;
    const uint32_t *stage2, *dec, *pool;
    const uint64_t *comp_key;
    const uint32_t *comp_val;
    uint32_t n_comp;
};

constexpr uint32_t NORM_FORM_NFC = 1, NORM_FORM_NFKC = 2;                 // KGPU_NORMALIZE_NFC / _NFKC
constexpr uint32_t NORM_MAX_SEGMENT = 64;                                  // KGPU_NORMALIZE_MAX_SEGMENT
constexpr uint32_t NORM_BUF = NORM_MAX_SEGMENT + 1;                        // a segment's first code point and that many more
constexpr uint32_t NORM_OVERSIZE = 0xFFFFFFFFu;
constexpr uint32_t NORM_MAX_EXPANSION = 11;                                // output bytes per input byte at most (U+FDFA: 3 -> 33)
constexpr uint32_t NORM_SBASE = 0xAC00, NORM_LBASE = 0x1100, NORM_VBASE = 0x1161, NORM_TBASE = 0x11A7, NORM_LCOUNT = 19, NORM_VCOUNT = 21, NORM_TCOUNT = 28,
                   NORM_NCOUNT = NORM_VCOUNT * NORM_TCOUNT, NORM_SCOUNT = NORM_LCOUNT * NORM_NCOUNT;

KGPU_NORM_HD uint32_t norm_props(const NormTables &t, uint32_t cp) {            // cp < 0x110000
    return t.stage2[(uint32_t)t.stage1[cp >> 7] * 128u + (cp & 127u)];
}
KGPU_NORM_HD bool norm_boundary(uint32_t props, uint32_t form) { return (props >> (form == NORM_FORM_NFC ? 8 : 10)) & 1u; }
KGPU_NORM_HD bool norm_inert(uint32_t props, uint32_t form) { return (props >> (form == NORM_FORM_NFC ? 9 : 11)) & 1u; }

// The sequence that starts at p (p < end): its length (1 where it is no valid sequence, so that a walk always advances) and its code point (below
// 0x110000 whatever the bytes are).  ok: a complete, shortest-form sequence of a scalar value -- what Rust's &str and Python's strict decoder accept.
KGPU_NORM_HD uint32_t norm_decode(const uint8_t *s, uint32_t p, uint32_t end, uint32_t &cp, bool &ok) {
    const uint32_t b = s[p];
    uint32_t l, lo;
    if (b < 0x80) { cp = b; ok = true; return 1; }
    if (b >= 0xC2 && b <= 0xDF) { l = 2; cp = b & 0x1Fu; lo = 0x80; }
    else if ((b & 0xF0u) == 0xE0u) { l = 3; cp = b & 0x0Fu; lo = 0x800; }
    else if (b >= 0xF0 && b <= 0xF4) { l = 4; cp = b & 0x07u; lo = 0x10000; }
    else { cp = 0xFFFD; ok = false; return 1; }
    ok = p + l <= end;
    if (ok)
        for (uint32_t j = 1; j < l; ++j) {
            const uint32_t bb = s[p + j];
            if ((bb & 0xC0u) != 0x80u) ok = false;
            cp = (cp << 6) | (bb & 0x3Fu);
        }
    if (ok && (cp < lo || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu))) ok = false;
    if (!ok) { cp = 0xFFFD; return 1; }
    return l;
}

KGPU_NORM_HD uint32_t norm_utf8_len(uint32_t cp) { return cp < 0x80 ? 1u : cp < 0x800 ? 2u : cp < 0x10000 ? 3u : 4u; }
// byte j (j < norm_utf8_len(cp)) of cp's encoding
KGPU_NORM_HD uint8_t norm_utf8_byte(uint32_t cp, uint32_t j) {
    const uint32_t l = norm_utf8_len(cp);
    if (l == 1) return (uint8_t)cp;
    const uint32_t shift = 6u * (l - 1 - j);
    if (j) return (uint8_t)(0x80u | ((cp >> shift) & 0x3Fu));
    return (uint8_t)((l == 2 ? 0xC0u : l == 3 ? 0xE0u : 0xF0u) | (cp >> shift));
}

// does the code point that starts at p (p < end) have a boundary before it?
KGPU_NORM_HD bool norm_boundary_at(const NormTables &t, uint32_t form, const uint8_t *s, uint32_t p, uint32_t end) {
    uint32_t cp;
    bool ok;
    (void)norm_decode(s, p, end, cp, ok);
    return norm_boundary(norm_props(t, cp), form);
}

// first + second -> the composite, or 0 (no code point composes to U+0000)
KGPU_NORM_HD uint32_t norm_compose(const NormTables &t, uint32_t a, uint32_t b) {
    if (a - NORM_LBASE < NORM_LCOUNT && b - NORM_VBASE < NORM_VCOUNT) return NORM_SBASE + ((a - NORM_LBASE) * NORM_VCOUNT + (b - NORM_VBASE)) * NORM_TCOUNT;
    if (a - NORM_SBASE < NORM_SCOUNT && (a - NORM_SBASE) % NORM_TCOUNT == 0 && b - (NORM_TBASE + 1) < NORM_TCOUNT - 1) return a + (b - NORM_TBASE);
    const uint64_t key = (uint64_t)a << 21 | b;
    uint32_t lo = 0, hi = t.n_comp;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.comp_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < t.n_comp && t.comp_key[lo] == key ? t.comp_val[lo] : 0u;
}

// One segment: the code points from p up to the next boundary or the line's end (the code point at p belongs to it whatever it is), decomposed under
// the form, put into canonical order and composed, left in buf[0 .. n).  Buf: get(i) / set(i, v) over NORM_BUF entries.  -> the UTF-8 bytes of the
// result, or NORM_OVERSIZE when the decomposition does not fit (buf's contents are then unspecified); next: where the segment ends.
template <class Buf>
KGPU_NORM_HD uint32_t norm_segment(const NormTables &t, uint32_t form, const uint8_t *s, uint32_t p, uint32_t end, Buf &buf, uint32_t &n, uint32_t &next) {
    uint32_t m = 0;
    bool over = false;
    do {
        uint32_t cp;
        bool ok;
        p += norm_decode(s, p, end, cp, ok);
        const uint32_t w = norm_props(t, cp);
        if (w & (1u << 12)) {   // a Hangul syllable: L V [T]
            const uint32_t si = cp - NORM_SBASE, ti = si % NORM_TCOUNT, cnt = ti ? 3u : 2u;
            if (m + cnt > NORM_BUF) { over = true; break; }
            buf.set(m++, NORM_LBASE + si / NORM_NCOUNT);
            buf.set(m++, NORM_VBASE + (si % NORM_NCOUNT) / NORM_TCOUNT);
            if (ti) buf.set(m++, NORM_TBASE + ti);
            continue;
        }
        const uint32_t k = w >> 13;
        const uint32_t d = k ? t.dec[2 * (k - 1) + (form == NORM_FORM_NFC ? 0 : 1)] : 0u;
        const uint32_t cnt = d & 0xFFu;
        if (m + (cnt ? cnt : 1u) > NORM_BUF) { over = true; break; }
        if (cnt == 0) buf.set(m++, cp | (w & 0xFFu) << 24);
        else for (uint32_t j = 0; j < cnt; ++j) buf.set(m++, t.pool[(d >> 8) + j]);
    } while (p < end && !norm_boundary_at(t, form, s, p, end));
    if (over) {   // (the segment's end is still found: the caller may want it)
        while (p < end && !norm_boundary_at(t, form, s, p, end)) {
            uint32_t c; bool ok;
            p += norm_decode(s, p, end, c, ok);
        }
        next = p; n = 0;
        return NORM_OVERSIZE;
    }
    next = p;
    // canonical order: a stable sort of every run of non-starters by combining class (insertion sort: the runs are short)
    for (uint32_t i = 1; i < m; ++i) {
        const uint32_t v = buf.get(i), cc = v >> 24;
        if (cc == 0) continue;
        uint32_t j = i;
        while (j > 0 && (buf.get(j - 1) >> 24) > cc) { buf.set(j, buf.get(j - 1)); --j; }
        if (j != i) buf.set(j, v);
    }
    // composition (UAX #15): a code point combines with the last starter unless a code point of its own or a higher class, or another starter, stands between
    uint32_t out = 0, starter = NORM_OVERSIZE, last_cc = 0, bytes = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t v = buf.get(i), c = v & 0x1FFFFFu, cc = v >> 24;
        if (starter != NORM_OVERSIZE && (last_cc < cc || last_cc == 0)) {
            const uint32_t comp = norm_compose(t, buf.get(starter) & 0x1FFFFFu, c);
            if (comp) { buf.set(starter, comp); continue; }
        }
        if (cc == 0) starter = out;
        last_cc = cc;
        buf.set(out++, v);
    }
    for (uint32_t i = 0; i < out; ++i) bytes += norm_utf8_len(buf.get(i) & 0x1FFFFFu);
    n = out;
    return bytes;
}

// The alignment of one walked segment (include/kanpyo_gpu.h, "source alignment"): a segment s[p .. next) that norm_segment left in buf[0 .. n) as `bytes`
// bytes of UTF-8 gives an edit exactly when those bytes are not the source's.  Its four lengths: out_len = bytes and out_chars = n (norm_segment's), and
// the source's, counted here (a code point is a byte that is no continuation byte: the line is UTF-8, or it has no edits).
struct NormSegEdit { uint32_t out_len, src_len, out_chars, src_chars; bool differs; };
template <class Buf>
KGPU_NORM_HD NormSegEdit norm_segment_edit(const uint8_t *s, uint32_t p, uint32_t next, const Buf &buf, uint32_t n, uint32_t bytes) {
    NormSegEdit e{bytes, next - p, n, 0, bytes != next - p};
    for (uint32_t q = p; q < next; ++q) e.src_chars += (s[q] & 0xC0u) != 0x80u;
    if (!e.differs)
        for (uint32_t i = 0, q = p; i < n; ++i) {
            const uint32_t c = buf.get(i) & 0x1FFFFFu, cl = norm_utf8_len(c);
            for (uint32_t j = 0; j < cl; ++j, ++q)
                if (norm_utf8_byte(c, j) != s[q]) e.differs = true;
        }
    return e;
}

}  // namespace kgpu
