// kanpyo_amd/csrc/kgpu_features.cpp -- the display tables behind the `kanpyo tokenize` output (reference src/bin/kanpyo.rs:174-197).
//
// Owns: the bincode 2 (standard config) parser of MorphFeatureTable (kanpyo-dict/src/morph_feature.rs:6-37) with the validation that turns
// the reference's print-time panics into KGPU_ERR_BAD_DICT, the pre-joined feature pool and its upload (kgpu_dict_set_features), the
// label pool of the graphviz node lines (src/graphviz.rs:56-89) and its upload on the first graphviz call (ensure_label_pool), the
// host-only test hooks over them (kgpu_debug_feature_pool, kgpu_debug_label_pool), the per-row word table of a words handle
// (build_word_table: field, fallback to the surface and filter decided per row; kgpu_words_host.cpp uploads it), and the CLI's line
// splitting (kgpu_split_lines: read_line + trim_end).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "kgpu_runtime.h"

namespace {

// bincode 2, config::standard(): unsigned integers as varints -- < 251 one byte, else a tag (251: u16, 252: u32, 253: u64, 254: u128)
// and the value little endian.  A tag wider than the decoded type, and tag 255, fail the decode (as do truncation and bad UTF-8).
struct Bin {
    const uint8_t *p; size_t n, at = 0;
    const char *err = nullptr;
    size_t left() const { return n - at; }
    bool var(uint64_t &v, int max_tag) {
        if (at >= n) { err = "truncated"; return false; }
        const uint8_t t = p[at++];
        if (t < 251) { v = t; return true; }
        if (t == 255) { err = "integer tag 255"; return false; }
        if (t > max_tag) { err = "integer tag wider than its type"; return false; }
        const size_t w = t == 251 ? 2 : t == 252 ? 4 : 8;
        if (left() < w) { err = "truncated"; return false; }
        v = 0;
        for (size_t k = 0; k < w; ++k) v |= (uint64_t)p[at + k] << (8 * k);
        at += w;
        return true;
    }
    bool len(uint64_t &v) { return var(v, 253); }   // usize -> u64
    bool u32(uint32_t &v) { uint64_t x; if (!var(x, 252)) return false; v = (uint32_t)x; return true; }
};

// Rust's str::from_utf8: shortest forms only, no surrogates, nothing above U+10FFFF.
bool valid_utf8(const uint8_t *s, size_t n) {
    for (size_t i = 0; i < n;) {
        const uint8_t c = s[i];
        if (c < 0x80) { ++i; continue; }
        size_t w; uint32_t lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) w = 2;
        else if (c >= 0xE0 && c <= 0xEF) { w = 3; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
        else if (c >= 0xF0 && c <= 0xF4) { w = 4; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
        else return false;
        if (n - i < w || s[i + 1] < lo || s[i + 1] > hi) return false;
        for (size_t k = 2; k < w; ++k) if ((s[i + k] & 0xC0) != 0x80) return false;
        i += w;
    }
    return true;
}

struct Table {
    std::vector<uint64_t> row;    // rows + 1 offsets into ids
    std::vector<uint32_t> ids;
    std::vector<uint64_t> name;   // names + 1 offsets into `bytes`
    std::vector<uint8_t> bytes;
};

int parse_table(const uint8_t *p, size_t n, Table &t, const char *what) {
    Bin r{p, n};
    uint64_t rows = 0, names = 0;
    auto fail = [&]() {
        kgpu::set_error("%s: bincode decode fails (%s at byte %zu): the reference's Dict::load would (kanpyo-dict/src/morph_feature.rs:28-37)", what, r.err, r.at);
        return KGPU_ERR_BAD_DICT;
    };
    if (!r.len(rows)) return fail();
    if (rows > r.left()) { r.err = "truncated"; return fail(); }   // every row takes a byte at least
    t.row.assign(1, 0);
    t.row.reserve((size_t)rows + 1);
    for (uint64_t i = 0; i < rows; ++i) {
        uint64_t k = 0;
        if (!r.len(k)) return fail();
        if (k > r.left()) { r.err = "truncated"; return fail(); }
        for (uint64_t j = 0; j < k; ++j) {
            uint32_t id = 0;
            if (!r.u32(id)) return fail();
            t.ids.push_back(id);
        }
        t.row.push_back(t.ids.size());
    }
    if (!r.len(names)) return fail();
    if (names > r.left()) { r.err = "truncated"; return fail(); }
    t.name.assign(1, 0);
    t.name.reserve((size_t)names + 1);
    for (uint64_t i = 0; i < names; ++i) {
        uint64_t len = 0;
        if (!r.len(len)) return fail();
        if (len > r.left()) { r.err = "truncated"; return fail(); }
        if (!valid_utf8(p + r.at, (size_t)len)) { r.err = "a name that is not UTF-8"; return fail(); }
        t.bytes.insert(t.bytes.end(), p + r.at, p + r.at + len);
        r.at += (size_t)len;
        t.name.push_back(t.bytes.size());
    }
    return KGPU_OK;   // (trailing bytes are ignored, as decode_from_slice ignores them)
}

// The first `need` rows of t (the rows the tokens of a dictionary with `need` morphs can name), each joined with ',', appended to pool; one
// offset per row appended to off.  A feature id past name_list in one of them is what the reference would panic on printing it.
int join_rows(const Table &t, uint64_t need, const char *what, const char *ref_line, std::vector<uint8_t> &pool, std::vector<uint32_t> &off) {
    const uint64_t rows = t.row.size() - 1, names = t.name.size() - 1;
    if (rows < need) {
        kgpu::set_error("%s: %llu feature rows for %llu morphs (the reference would panic printing a token: src/bin/kanpyo.rs:178-186, morph_features[id - 1])",
                        what, (unsigned long long)rows, (unsigned long long)need);
        return KGPU_ERR_BAD_DICT;
    }
    for (uint64_t i = 0; i < t.row[need]; ++i)   // the rows a token can name (rows past them are never printed: kanpyo.rs:178-188)
        if (t.ids[i] >= names) {
            kgpu::set_error("%s: feature id %u, name_list has %llu names (the reference would panic printing it: src/bin/kanpyo.rs:%s)", what, t.ids[i],
                            (unsigned long long)names, ref_line);
            return KGPU_ERR_BAD_DICT;
        }
    for (uint64_t r = 0; r < need; ++r) {
        uint64_t size = pool.size();
        for (uint64_t j = t.row[r]; j < t.row[r + 1]; ++j) size += (j > t.row[r]) + (t.name[t.ids[j] + 1] - t.name[t.ids[j]]);
        if (size >= (1ull << 32)) { kgpu::set_error("%s: the joined feature strings reach 4 GiB", what); return KGPU_ERR_BAD_DICT; }
        for (uint64_t j = t.row[r]; j < t.row[r + 1]; ++j) {
            if (j > t.row[r]) pool.push_back(',');
            pool.insert(pool.end(), t.bytes.begin() + (ptrdiff_t)t.name[t.ids[j]], t.bytes.begin() + (ptrdiff_t)t.name[t.ids[j] + 1]);
        }
        off.push_back((uint32_t)pool.size());
    }
    return KGPU_OK;
}

// The same rows as a graphviz node's label has them (src/graphviz.rs:56-89): the names equal to "*" dropped, the rest -- an empty name too --
// joined with '/'.  Behind join_rows, which has checked the rows: a label row is never longer than its ',' row.
void join_labels(const Table &t, uint64_t need, std::vector<uint8_t> &pool, std::vector<uint32_t> &off) {
    for (uint64_t r = 0; r < need; ++r) {
        bool first = true;
        for (uint64_t j = t.row[r]; j < t.row[r + 1]; ++j) {
            const uint64_t n0 = t.name[t.ids[j]], n1 = t.name[t.ids[j] + 1];
            if (n1 - n0 == 1 && t.bytes[(size_t)n0] == '*') continue;
            if (!first) pool.push_back('/');
            first = false;
            pool.insert(pool.end(), t.bytes.begin() + (ptrdiff_t)n0, t.bytes.begin() + (ptrdiff_t)n1);
        }
        off.push_back((uint32_t)pool.size());
    }
}

// Both tables -> the pool in the records' index space (kgpu_runtime.h: kgpu_dict::feat): known rows, then unknown rows.  lpool / loff: the label
// pool over the same rows (null: not wanted).
int build_pool(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
               std::vector<uint8_t> &pool, std::vector<uint32_t> &off, std::vector<uint8_t> *lpool = nullptr, std::vector<uint32_t> *loff = nullptr) {
    Table tk, tu;
    int rc;
    if ((rc = parse_table(known, known_len, tk, "morph_feature.dict")) || (rc = parse_table(unk, unk_len, tu, "unk.dict feature table"))) return rc;
    off.assign(1, 0);
    off.reserve((size_t)(n_morphs + n_unk + 1));
    if ((rc = join_rows(tk, n_morphs, "morph_feature.dict", "181", pool, off)) || (rc = join_rows(tu, n_unk, "unk.dict feature table", "188", pool, off)))
        return rc;
    if (lpool) {
        loff->assign(1, 0);
        loff->reserve((size_t)(n_morphs + n_unk + 1));
        join_labels(tk, n_morphs, *lpool, *loff);
        join_labels(tu, n_unk, *lpool, *loff);
    }
    return KGPU_OK;
}

// One table's first `need` rows -> their word entries, appended to `rows`; the names they select go into `pool` once each (`seen`).
int word_rows(const Table &t, uint64_t need, const char *what, const kgpu_words_spec &spec, const std::unordered_set<std::string> &listed,
              std::unordered_map<std::string, uint32_t> &seen, std::vector<WordRow> &rows, std::vector<uint8_t> &pool) {
    const uint64_t n_rows = t.row.size() - 1, names = t.name.size() - 1;
    if (n_rows < need) {
        kgpu::set_error("%s: %llu feature rows for %llu morphs", what, (unsigned long long)n_rows, (unsigned long long)need);
        return KGPU_ERR_BAD_DICT;
    }
    const auto name_of = [&](uint32_t id) { return std::string(t.bytes.begin() + (ptrdiff_t)t.name[id], t.bytes.begin() + (ptrdiff_t)t.name[id + 1]); };
    for (uint64_t r = 0; r < need; ++r) {
        const uint64_t j0 = t.row[r], k = t.row[r + 1] - j0;
        for (uint64_t j = j0; j < j0 + k; ++j)
            if (t.ids[j] >= names) { kgpu::set_error("%s: feature id %u, name_list has %llu names", what, t.ids[j], (unsigned long long)names); return KGPU_ERR_BAD_DICT; }
        WordRow e{0, WORD_SURFACE};
        // the filter: feature 0 against the list; a row without features matches no name
        const bool match = spec.filter != KGPU_WORDS_ALL && k > 0 && listed.count(name_of(t.ids[j0])) != 0;
        if ((spec.filter == KGPU_WORDS_DROP && match) || (spec.filter == KGPU_WORDS_KEEP && !match)) e.len_flags |= WORD_DROPPED;
        // the word: feature `field`, unless the row is too short for it or it is "" or "*" (then the surface)
        if (spec.field >= 0 && (uint64_t)spec.field < k) {
            const std::string nm = name_of(t.ids[j0 + (uint64_t)spec.field]);
            if (!nm.empty() && nm != "*") {
                if (nm.size() > WORD_LEN_MASK) { kgpu::set_error("%s: a name of %zu bytes", what, nm.size()); return KGPU_ERR_BAD_DICT; }
                auto it = seen.find(nm);
                if (it == seen.end()) {
                    if (pool.size() + nm.size() >= (1ull << 32)) { kgpu::set_error("%s: the distinct names of field %d reach 4 GiB", what, spec.field); return KGPU_ERR_BAD_DICT; }
                    it = seen.emplace(nm, (uint32_t)pool.size()).first;
                    pool.insert(pool.end(), nm.begin(), nm.end());
                }
                e.off = it->second;
                e.len_flags = (e.len_flags & WORD_DROPPED) | (uint32_t)nm.size();
            }
        }
        rows.push_back(e);
    }
    return KGPU_OK;
}

}  // namespace

int kgpu::build_word_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                           const kgpu_words_spec &spec, std::vector<WordRow> &rows, std::vector<uint8_t> &names) {
    Table tk, tu;
    int rc;
    if ((rc = parse_table(known, known_len, tk, "morph_feature.dict")) || (rc = parse_table(unk, unk_len, tu, "unk.dict feature table"))) return rc;
    std::unordered_set<std::string> listed;
    for (uint64_t i = 0; i < spec.n_names; ++i) listed.emplace((const char *)spec.names + spec.name_offsets[i], (size_t)(spec.name_offsets[i + 1] - spec.name_offsets[i]));
    std::unordered_map<std::string, uint32_t> seen;
    rows.clear(); names.clear();
    rows.reserve((size_t)(n_morphs + n_unk));
    if ((rc = word_rows(tk, n_morphs, "morph_feature.dict", spec, listed, seen, rows, names)) ||
        (rc = word_rows(tu, n_unk, "unk.dict feature table", spec, listed, seen, rows, names)))
        return rc;
    return KGPU_OK;
}

extern "C" int kgpu_dict_set_features(kgpu_dict *d, const uint8_t *morph_feature_dict, size_t morph_feature_len,
                                      const uint8_t *unk_feature_dict, size_t unk_feature_len) {
    if (!d || (morph_feature_len && !morph_feature_dict) || (unk_feature_len && !unk_feature_dict)) {
        set_error("kgpu_dict_set_features: null argument");
        return KGPU_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> g(d->feat_mu);
    if (d->feat) { set_error("kgpu_dict_set_features: the handle has its feature tables already (once per handle)"); return KGPU_ERR_INVALID_ARG; }
    std::vector<uint8_t> pool;
    std::vector<uint32_t> off;
    std::vector<uint8_t> lpool;
    std::vector<uint32_t> loff;
    int rc = build_pool(morph_feature_dict, morph_feature_len, unk_feature_dict, unk_feature_len, d->info.n_morphs, d->info.n_unk_morphs, pool, off, &lpool, &loff);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(d->device));
    void *dp = nullptr, *doff = nullptr;
    const size_t pool_bytes = std::max<size_t>(pool.size(), 16), off_bytes = off.size() * sizeof(uint32_t);
    HIPCHECK(hipMalloc(&dp, pool_bytes));
    d->allocs.push_back(dp);
    HIPCHECK(hipMalloc(&doff, off_bytes));
    d->allocs.push_back(doff);
    if (!pool.empty()) HIPCHECK(hipMemcpy(dp, pool.data(), pool.size(), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(doff, off.data(), off_bytes, hipMemcpyHostToDevice));
    d->info.device_bytes += pool_bytes + off_bytes;
    d->feat = (const uint8_t *)dp;
    d->feat_off = (const uint32_t *)doff;
    d->label_host.swap(lpool);   // stays on the host until a lattice is drawn (ensure_label_pool)
    d->label_off_host.swap(loff);
    d->feat_blob_known.assign(morph_feature_dict, morph_feature_dict + morph_feature_len);   // what a later kgpu_words_create parses
    d->feat_blob_unk.assign(unk_feature_dict, unk_feature_dict + unk_feature_len);
    return KGPU_OK;
}

// The label pool on the device, uploaded by the first graphviz call of the handle (behind require_features).
int kgpu::ensure_label_pool(kgpu_dict *d) {
    std::lock_guard<std::mutex> g(d->feat_mu);
    if (d->label) return KGPU_OK;
    HIPCHECK(hipSetDevice(d->device));
    void *dp = nullptr, *doff = nullptr;
    const size_t pool_bytes = std::max<size_t>(d->label_host.size(), 16), off_bytes = d->label_off_host.size() * sizeof(uint32_t);
    HIPCHECK(hipMalloc(&dp, pool_bytes));
    d->allocs.push_back(dp);
    HIPCHECK(hipMalloc(&doff, off_bytes));
    d->allocs.push_back(doff);
    if (!d->label_host.empty()) HIPCHECK(hipMemcpy(dp, d->label_host.data(), d->label_host.size(), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(doff, d->label_off_host.data(), off_bytes, hipMemcpyHostToDevice));
    d->info.device_bytes += pool_bytes + off_bytes;
    d->label_off = (const uint32_t *)doff;
    d->label = (const uint8_t *)dp;
    return KGPU_OK;
}

// Test hook (host only, not in the header): the parser, the validation and the pool of kgpu_dict_set_features without a device.
// offsets: n_morphs + n_unk + 1 entries.  KGPU_ERR_CAPACITY: pool_cap < *pool_len.
extern "C" int kgpu_debug_feature_pool(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                                       uint8_t *pool, uint64_t pool_cap, uint32_t *offsets, uint64_t *pool_len) {
    std::vector<uint8_t> p;
    std::vector<uint32_t> off;
    const int rc = build_pool(known, known_len, unk, unk_len, n_morphs, n_unk, p, off);
    if (rc) return rc;
    if (pool_len) *pool_len = p.size();
    if (offsets) std::memcpy(offsets, off.data(), off.size() * sizeof(uint32_t));
    if (p.size() > pool_cap) { set_error("pool buffer too small: need %zu", p.size()); return KGPU_ERR_CAPACITY; }
    if (!p.empty()) std::memcpy(pool, p.data(), p.size());
    return KGPU_OK;
}

// ... and the label pool of the same tables (offsets: n_morphs + n_unk + 1 entries; the validation is kgpu_debug_feature_pool's).
extern "C" int kgpu_debug_label_pool(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                                     uint8_t *pool, uint64_t pool_cap, uint32_t *offsets, uint64_t *pool_len) {
    std::vector<uint8_t> p, lp;
    std::vector<uint32_t> off, loff;
    const int rc = build_pool(known, known_len, unk, unk_len, n_morphs, n_unk, p, off, &lp, &loff);
    if (rc) return rc;
    if (pool_len) *pool_len = lp.size();
    if (offsets) std::memcpy(offsets, loff.data(), loff.size() * sizeof(uint32_t));
    if (lp.size() > pool_cap) { set_error("pool buffer too small: need %zu", lp.size()); return KGPU_ERR_CAPACITY; }
    if (!lp.empty()) std::memcpy(pool, lp.data(), lp.size());
    return KGPU_OK;
}

// The Unicode White_Space code points (what Rust's str::trim_end strips, char::is_whitespace) ending at s[0 .. n): their byte length, 0 if none.
static size_t trailing_space(const uint8_t *s, size_t n) {
    if (n == 0) return 0;
    const uint8_t c = s[n - 1];
    if ((c >= 0x09 && c <= 0x0D) || c == 0x20) return 1;
    if (n >= 2 && s[n - 2] == 0xC2 && (c == 0x85 || c == 0xA0)) return 2;                     // U+0085, U+00A0
    if (n < 3) return 0;
    const uint8_t a = s[n - 3], b = s[n - 2];
    if (a == 0xE1 && b == 0x9A && c == 0x80) return 3;                                        // U+1680
    if (a == 0xE2 && b == 0x80 && (c <= 0x8A || c == 0xA8 || c == 0xA9 || c == 0xAF) && c >= 0x80) return 3;   // U+2000-200A, 2028, 2029, 202F
    if (a == 0xE2 && b == 0x81 && c == 0x9F) return 3;                                        // U+205F
    if (a == 0xE3 && b == 0x80 && c == 0x80) return 3;                                        // U+3000
    return 0;
}

extern "C" int kgpu_split_lines(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t *offsets, uint64_t offsets_capacity, uint64_t *n_lines) {
    if ((len && (!in || !out)) || !n_lines || (offsets_capacity && !offsets)) { set_error("kgpu_split_lines: null argument"); return KGPU_ERR_INVALID_ARG; }
    uint64_t lines = 0;
    for (uint64_t i = 0; i < len; ++i) lines += in[i] == '\n';
    if (len && in[len - 1] != '\n') ++lines;   // a last line without its newline
    *n_lines = lines;
    if (offsets_capacity < lines + 1) {
        set_error("kgpu_split_lines: offsets capacity %llu, need %llu", (unsigned long long)offsets_capacity, (unsigned long long)(lines + 1));
        return KGPU_ERR_CAPACITY;
    }
    uint64_t at = 0, o = 0, k = 0;
    offsets[0] = 0;
    while (at < len) {
        const uint8_t *nl = (const uint8_t *)memchr(in + at, '\n', (size_t)(len - at));
        const uint64_t end = nl ? (uint64_t)(nl - in) : len;
        size_t m = (size_t)(end - at), t;
        while ((t = trailing_space(in + at, m)) != 0) m -= t;
        std::memmove(out + o, in + at, m);   // (out may be `in` itself: the packed lines never overtake the input)
        o += m;
        offsets[++k] = o;
        at = end + 1;
    }
    return KGPU_OK;
}
