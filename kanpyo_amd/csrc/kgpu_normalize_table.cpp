// kanpyo_amd/csrc/kgpu_normalize_table.cpp -- the tables of the text normaliser (include/kanpyo_gpu.h, "text normalisation"; generated:
// kgpu_normalize_data.inc) and the normaliser itself on the host: kgpu_normalize_host, which every device result is defined to equal.  HIP-free: a plain
// C++ compiler builds this file alone (tests/c_abi/normalize_main.cpp).  kgpu_normalize_host.cpp uploads the same arrays; kgpu_normalize.hip runs the same
// segment code (kgpu_normalize_core.h) over them.
#include <cstring>
#include <vector>

#include "kgpu_align_core.h"
#include "kgpu_internal.h"
#include "kgpu_normalize_core.h"

namespace kgpu {

namespace {
#include "kgpu_normalize_data.inc"
}  // namespace

static_assert(KGPU_NORMALIZE_MAX_SEGMENT == NORM_MAX_SEGMENT && KGPU_NORMALIZE_NFC == NORM_FORM_NFC && KGPU_NORMALIZE_NFKC == NORM_FORM_NFKC, "header and core agree");

// The committed file is compact (tools/gen_normalize_tables.py: build_tables); the tables of kgpu_normalize_core.h are made from it once, when first asked for.
struct Expanded {
    std::vector<uint16_t> stage1;
    std::vector<uint32_t> stage2, dec, pool;
    Expanded() {
        constexpr uint32_t N_RUNS = sizeof NORM_RUN_START / sizeof NORM_RUN_START[0], N_DEC = sizeof NORM_DEC_STEP / sizeof NORM_DEC_STEP[0], LAST = 0x110000;
        std::vector<uint32_t> word(LAST);
        for (uint32_t r = 0; r < N_RUNS; ++r)
            for (uint32_t cp = NORM_RUN_START[r], end = r + 1 < N_RUNS ? NORM_RUN_START[r + 1] : LAST; cp < end; ++cp) word[cp] = NORM_RUN_BITS[r];
        pool.assign(NORM_POOL_CP, NORM_POOL_CP + sizeof NORM_POOL_CP / sizeof NORM_POOL_CP[0]);
        for (uint32_t &c : pool) c |= (word[c] & 0xFFu) << 24;   // a pool entry carries its combining class
        dec.reserve(2 * (size_t)N_DEC);
        for (uint32_t k = 0, cp = 0; k < N_DEC; ++k) {
            cp += NORM_DEC_STEP[k];
            word[cp] |= (k + 1) << 13;
            dec.push_back(NORM_DEC_NFD[k]);
            dec.push_back(NORM_DEC_NFKD[k]);
        }
        stage1.resize(LAST / 128);
        for (uint32_t b = 0; b < LAST / 128; ++b) {   // equal blocks of 128 words are stored once (a few hundred distinct ones: a linear search does)
            uint32_t at = 0;
            const uint32_t have = (uint32_t)(stage2.size() / 128);
            while (at < have && std::memcmp(&stage2[(size_t)at * 128], &word[(size_t)b * 128], 128 * 4) != 0) ++at;
            if (at == have) stage2.insert(stage2.end(), word.begin() + (size_t)b * 128, word.begin() + (size_t)(b + 1) * 128);
            stage1[b] = (uint16_t)at;
        }
    }
};
static const Expanded &expanded() {
    static const Expanded e;
    return e;
}

NormTables norm_host_tables() {
    const Expanded &e = expanded();
    return NormTables{e.stage1.data(), e.stage2.data(), e.dec.data(), e.pool.data(), NORM_COMP_KEY, NORM_COMP_VAL, (uint32_t)(sizeof NORM_COMP_VAL / sizeof NORM_COMP_VAL[0])};
}
NormTableSizes norm_table_sizes() {
    const Expanded &e = expanded();
    return NormTableSizes{e.stage1.size() * 2, e.stage2.size() * 4, e.dec.size() * 4, e.pool.size() * 4, sizeof NORM_COMP_KEY, sizeof NORM_COMP_VAL};
}

namespace {

struct HostBuf {
    uint32_t v[NORM_BUF];
    uint32_t get(uint32_t i) const { return v[i]; }
    void set(uint32_t i, uint32_t x) { v[i] = x; }
};

// One pass over a line: its normalised length and the number of its edits ("source alignment"), and with `out` the bytes, with `edits` the records.
// -> the status; the length is the line's own and there are no edits when the status is not 0.
uint8_t pass(const NormTables &t, uint32_t form, const uint8_t *s, uint32_t len, uint8_t *out, uint64_t &out_len, kgpu_norm_edit *edits, uint64_t &n_edits) {
    out_len = len;
    n_edits = 0;
    for (uint32_t p = 0; p < len;) {
        uint32_t cp;
        bool ok;
        p += norm_decode(s, p, len, cp, ok);
        if (!ok) return KGPU_SENT_INVALID_UTF8;
    }
    uint64_t o = 0, ne = 0;
    uint32_t oc = 0, sc = 0;   // code points written, code points read
    HostBuf buf;
    for (uint32_t p = 0; p < len;) {
        uint32_t cp;
        bool ok;
        const uint32_t l = norm_decode(s, p, len, cp, ok);
        const uint32_t w = norm_props(t, cp);
        if (norm_inert(w, form) && (p + l == len || norm_boundary_at(t, form, s, p + l, len))) {   // a segment of one inert code point: as it is
            if (out) std::memcpy(out + o, s + p, l);
            o += l; p += l;
            ++oc; ++sc;
            continue;
        }
        uint32_t n, next;
        const uint32_t bytes = norm_segment(t, form, s, p, len, buf, n, next);
        if (bytes == NORM_OVERSIZE) return KGPU_SENT_NOT_NORMALIZED;
        if (out)
            for (uint32_t i = 0, q = 0; i < n; ++i) {
                const uint32_t c = buf.get(i) & 0x1FFFFFu, cl = norm_utf8_len(c);
                for (uint32_t j = 0; j < cl; ++j) out[o + q++] = norm_utf8_byte(c, j);
            }
        const NormSegEdit e = norm_segment_edit(s, p, next, buf, n, bytes);
        if (e.differs) {
            if (edits) edits[ne] = kgpu_norm_edit{(uint32_t)o, p, oc, sc, (uint16_t)e.out_len, (uint16_t)e.src_len, (uint16_t)e.out_chars, (uint16_t)e.src_chars};
            ++ne;
        }
        oc += e.out_chars; sc += e.src_chars;
        o += bytes; p = next;
    }
    out_len = o;
    n_edits = ne;
    return KGPU_SENT_OK;
}

}  // namespace

uint8_t norm_line_host(uint32_t form, const uint8_t *s, uint32_t len, uint8_t *out, uint64_t capacity, uint64_t &out_len) {
    uint64_t n_edits;
    return norm_line_host_aligned(form, s, len, out, capacity, out_len, nullptr, ~0ull, n_edits);
}
uint8_t norm_line_host_aligned(uint32_t form, const uint8_t *s, uint32_t len, uint8_t *out, uint64_t capacity, uint64_t &out_len, kgpu_norm_edit *edits,
                               uint64_t edit_capacity, uint64_t &n_edits) {
    const NormTables t = norm_host_tables();
    const uint8_t st = pass(t, form, s, len, nullptr, out_len, nullptr, n_edits);
    if (out_len > capacity || n_edits > edit_capacity) return st;
    if (st != KGPU_SENT_OK) { if (len) std::memcpy(out, s, len); return st; }
    uint64_t again, edits_again;
    (void)pass(t, form, s, len, out, again, edits, edits_again);
    return st;
}

}  // namespace kgpu

extern "C" const char *kgpu_normalize_unicode_version(void) { return KGPU_NORM_UNIDATA; }

extern "C" int kgpu_normalize_host(int form, const uint8_t *in, uint64_t len, uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint8_t *status) {
    if ((form != KGPU_NORMALIZE_NFC && form != KGPU_NORMALIZE_NFKC) || (len && !in) || (capacity && !out) || !n_bytes) {
        kgpu::set_error("kgpu_normalize_host: null argument or unknown form");
        return KGPU_ERR_INVALID_ARG;
    }
    *n_bytes = 0;
    if (len >= (1ull << 32)) { kgpu::set_error("kgpu_normalize_host: a string of 4 GiB or more"); return KGPU_ERR_INVALID_ARG; }
    uint64_t need = 0;
    const uint8_t st = kgpu::norm_line_host((uint32_t)form, in, (uint32_t)len, out, capacity, need);
    *n_bytes = need;
    if (status) *status = st;
    if (need > capacity) {
        kgpu::set_error("kgpu_normalize_host: buffer too small: need %llu, capacity %llu", (unsigned long long)need, (unsigned long long)capacity);
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}

extern "C" int kgpu_normalize_host_aligned(int form, const uint8_t *in, uint64_t len, uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint8_t *status,
                                           kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *n_edits) {
    if ((form != KGPU_NORMALIZE_NFC && form != KGPU_NORMALIZE_NFKC) || (len && !in) || (capacity && !out) || !n_bytes || (edit_capacity && !edits) || !n_edits) {
        kgpu::set_error("kgpu_normalize_host_aligned: null argument or unknown form");
        return KGPU_ERR_INVALID_ARG;
    }
    *n_bytes = 0; *n_edits = 0;
    if (len >= (1ull << 32)) { kgpu::set_error("kgpu_normalize_host_aligned: a string of 4 GiB or more"); return KGPU_ERR_INVALID_ARG; }
    uint64_t need = 0, need_edits = 0;
    const uint8_t st = kgpu::norm_line_host_aligned((uint32_t)form, in, (uint32_t)len, out, capacity, need, edits, edit_capacity, need_edits);
    *n_bytes = need; *n_edits = need_edits;
    if (status) *status = st;
    if (need > capacity || need_edits > edit_capacity) {
        kgpu::set_error("kgpu_normalize_host_aligned: buffers too small: need %llu bytes (capacity %llu) and %llu edits (capacity %llu)", (unsigned long long)need,
                        (unsigned long long)capacity, (unsigned long long)need_edits, (unsigned long long)edit_capacity);
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}

extern "C" void kgpu_source_spans_host(const kgpu_token *tokens, const uint64_t *tok_offsets, uint64_t n, const kgpu_norm_edit *edits,
                                       const uint64_t *edit_offsets, kgpu_span *spans) {
    for (uint64_t s = 0; s < n; ++s) {
        const uint64_t e0 = edit_offsets[s], e1 = edit_offsets[s + 1];
        for (uint64_t k = tok_offsets[s]; k < tok_offsets[s + 1]; ++k) spans[k - tok_offsets[0]] = kgpu::align_span(tokens[k], edits + e0, e1 > e0 ? e1 - e0 : 0);
    }
}
