// kanpyo_amd/csrc/kgpu_count_host.cpp -- the counts handle behind the word counts (include/kanpyo_gpu.h, "word counts"; kgpu_count.hip).
//
// Owns: kgpu_counts_create / _destroy / _reset / _get_info; the count's enqueue on a context (enqueue_count), kgpu_count_words_device and
// kgpu_ctx_sync_count; the host calls kgpu_count_batch and kgpu_count_text -- the lines calls' sources and records chunk (ChunkSource, RecordsChunk,
// kgpu_runtime.h) with a finish that counts (CountChunk) under one body (count_call); the read-out kgpu_counts_read with the dictionary's id -> key table behind it; and the host-only test hook
// kgpu_debug_counts_order (the merge and the order of the read-out without a device).
//
// ACCUMULATION IS NOT IDEMPOTENT.  The renders of a lines chunk are queued behind the chunk's first pass and simply run once more when kgpu_ctx_sync
// had to rerun the chain (LinesChunk::finish); a count cannot be taken back.  A count chunk's kernel is therefore enqueued only when kgpu_ctx_sync has
// returned -- the chunk's records are final then -- and waited for at once; the ring's other chunks keep the device busy meanwhile.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "kgpu_runtime.h"

namespace {

struct Entry { const uint8_t *p; uint64_t len, count; };

inline int cmp_bytes(const Entry &a, const Entry &b) {   // memcmp order; a proper prefix comes first
    const uint64_t m = std::min(a.len, b.len);
    const int c = m ? std::memcmp(a.p, b.p, (size_t)m) : 0;
    return c ? c : (a.len < b.len ? -1 : a.len > b.len ? 1 : 0);
}

// Rule 5: equal byte strings merged (their counts summed), ordered by count descending then bytes ascending, cut after `top` (0: not cut).
void merge_and_order(std::vector<Entry> &e, uint64_t top) {
    std::sort(e.begin(), e.end(), [](const Entry &a, const Entry &b) { return cmp_bytes(a, b) < 0; });
    size_t out = 0;
    for (size_t i = 0; i < e.size(); ++i) {
        if (out && cmp_bytes(e[out - 1], e[i]) == 0) e[out - 1].count += e[i].count;
        else e[out++] = e[i];
    }
    e.resize(out);
    std::stable_sort(e.begin(), e.end(), [](const Entry &a, const Entry &b) { return a.count > b.count; });   // (stable: ties stay in byte order)
    if (top && e.size() > top) e.resize((size_t)top);
}

// The entries into three flat arrays (what the handle caches and what the read-out hands over).
void flatten(const std::vector<Entry> &e, std::vector<uint8_t> &words, std::vector<uint64_t> &off, std::vector<uint64_t> &counts) {
    uint64_t bytes = 0;
    for (const Entry &x : e) bytes += x.len;
    words.resize((size_t)bytes); off.resize(e.size() + 1); counts.resize(e.size());
    uint64_t at = 0;
    for (size_t i = 0; i < e.size(); ++i) {
        off[i] = at; counts[i] = e[i].count;
        if (e[i].len) std::memcpy(words.data() + at, e[i].p, (size_t)e[i].len);
        at += e[i].len;
    }
    off[e.size()] = at;
}

// The exact-sizes protocol of the read-out.
int deliver(const char *who, const std::vector<uint8_t> &words, const std::vector<uint64_t> &off, const std::vector<uint64_t> &counts, uint64_t top,
            uint8_t *out_words, uint64_t words_capacity, uint64_t *word_offsets, uint64_t *out_counts, uint64_t entries_capacity, uint64_t *n_entries, uint64_t *n_bytes) {
    const uint64_t n = top && counts.size() > top ? top : counts.size(), bytes = off[(size_t)n];
    *n_entries = n; *n_bytes = bytes;
    if (n > entries_capacity || bytes > words_capacity) {
        set_error("%s: buffers too small: need %llu entries (capacity %llu) and %llu bytes (capacity %llu)", who, (unsigned long long)n,
                  (unsigned long long)entries_capacity, (unsigned long long)bytes, (unsigned long long)words_capacity);
        return KGPU_ERR_CAPACITY;
    }
    if ((n && (!word_offsets || !out_counts)) || (bytes && !out_words)) { set_error("%s: null output", who); return KGPU_ERR_INVALID_ARG; }
    if (bytes) std::memcpy(out_words, words.data(), (size_t)bytes);
    if (word_offsets) std::memcpy(word_offsets, off.data(), (size_t)(n + 1) * 8);
    if (n) std::memcpy(out_counts, counts.data(), (size_t)n * 8);
    return KGPU_OK;
}

int reset_device(kgpu_counts *k) {
    kgpu_dict *d = k->words->dict;
    HIPCHECK(hipSetDevice(d->device));
    const size_t rows = (size_t)(d->info.n_morphs + d->info.n_unk_morphs);
    HIPCHECK(hipMemset(k->d_dense, 0, std::max<size_t>(rows * 8, 16)));
    HIPCHECK(hipMemset(k->d_slots, 0, (size_t)k->table_slots * sizeof(CountSlot)));
    HIPCHECK(hipMemset(k->d_stats, 0, COUNT_STAT_WORDS * 8));
    HIPCHECK(hipDeviceSynchronize());
    return KGPU_OK;
}

void free_counts(kgpu_counts *k) {
    (void)hipSetDevice(k->words->dict->device);
    (void)hipFree(k->d_dense); (void)hipFree(k->d_slots); (void)hipFree(k->d_arena); (void)hipFree(k->d_stats);
    kgpu_words *w = k->words;
    delete k;
    words_release(w);
}

}  // namespace

// The dictionary's id -> key table, built by the first read-out or vocabulary handle that needs it (the double array as the caller gave it is released then).
void kgpu::dict_key_table(kgpu_dict *d) {
    std::lock_guard<std::mutex> g(d->keys_mu);
    if (d->keys_built) return;
    build_key_table(d->da_host, d->dup_host, d->info.n_morphs, d->key_bytes, d->key_off);
    std::vector<DaNode>().swap(d->da_host);
    std::vector<std::pair<int64_t, uint64_t>>().swap(d->dup_host);
    d->keys_built = true;
}

extern "C" int kgpu_counts_create(kgpu_words *w, const kgpu_counts_opts *opts, kgpu_counts **out) {
    const char *who = "kgpu_counts_create";
    if (!w || !out) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    uint64_t slots = KGPU_COUNTS_DEFAULT_SLOTS, key_bytes = KGPU_COUNTS_DEFAULT_KEY_BYTES;
    if (opts) {
        if (opts->size < sizeof(kgpu_counts_opts)) { set_error("%s: opts.size %u, the struct has %zu bytes", who, opts->size, sizeof(kgpu_counts_opts)); return KGPU_ERR_INVALID_ARG; }
        if (opts->table_slots) slots = opts->table_slots;
        if (opts->key_bytes) key_bytes = opts->key_bytes;
    }
    if (slots > (1ull << 32) || key_bytes > (1ull << 34)) { set_error("%s: at most 2^32 slots and 2^34 key bytes", who); return KGPU_ERR_INVALID_ARG; }
    uint64_t p2 = 1;
    while (p2 < slots) p2 <<= 1;
    slots = p2;
    key_bytes = (key_bytes + 7) & ~7ull;
    kgpu_dict *d = w->dict;
    HIPCHECK(hipSetDevice(d->device));
    kgpu_counts *k = new kgpu_counts();
    k->words = w;
    w->refs.fetch_add(1, std::memory_order_relaxed);
    k->table_slots = slots; k->key_bytes = key_bytes;
    const size_t rows = (size_t)(d->info.n_morphs + d->info.n_unk_morphs);
    if (hipMalloc(&k->d_dense, std::max<size_t>(rows * 8, 16)) != hipSuccess || hipMalloc(&k->d_slots, (size_t)slots * sizeof(CountSlot)) != hipSuccess ||
        hipMalloc(&k->d_arena, (size_t)key_bytes + 16) != hipSuccess || hipMalloc(&k->d_stats, COUNT_STAT_WORDS * 8) != hipSuccess) {
        (void)hipGetLastError();
        free_counts(k);
        set_error("%s: no device memory for %llu rows, %llu slots and %llu key bytes", who, (unsigned long long)rows, (unsigned long long)slots, (unsigned long long)key_bytes);
        return KGPU_ERR_HIP;
    }
    if (int rc = reset_device(k)) { free_counts(k); return rc; }
    *out = k;
    return KGPU_OK;
}

extern "C" void kgpu_counts_destroy(kgpu_counts *k) {
    if (k) free_counts(k);
}

extern "C" int kgpu_counts_reset(kgpu_counts *k) {
    if (!k) { set_error("kgpu_counts_reset: null handle"); return KGPU_ERR_INVALID_ARG; }
    std::unique_lock<std::shared_mutex> g(k->mu);
    k->version.fetch_add(1, std::memory_order_acq_rel);
    k->sentences.store(0, std::memory_order_relaxed);
    return reset_device(k);
}

extern "C" int kgpu_counts_get_info(kgpu_counts *k, kgpu_counts_info *info) {
    if (!k || !info || info->size < 8) { set_error("kgpu_counts_get_info: null argument, or info.size not set"); return KGPU_ERR_INVALID_ARG; }
    std::unique_lock<std::shared_mutex> g(k->mu);
    HIPCHECK(hipSetDevice(k->words->dict->device));
    unsigned long long st[COUNT_STAT_WORDS];
    HIPCHECK(hipMemcpy(st, k->d_stats, sizeof st, hipMemcpyDeviceToHost));
    kgpu_counts_info full{};
    full.size = (uint32_t)std::min<size_t>(info->size, sizeof full);
    full.tokens_counted = st[2]; full.overflow_tokens = st[3];
    full.sentences = k->sentences.load(std::memory_order_relaxed);
    full.table_slots = k->table_slots; full.table_slots_used = st[1];
    full.key_bytes = k->key_bytes; full.key_bytes_used = std::min<uint64_t>(st[0], k->key_bytes);
    std::memcpy(info, &full, full.size);
    return KGPU_OK;
}

// ---- the count of a batch's records on a context ---------------------------------------------------------------------------------------------
int kgpu::enqueue_count(kgpu_ctx *c, kgpu_counts *k, const DeviceRecords &r, const char *who) {
    if (k->words->dict != c->dict) { set_error("%s: the context's dictionary is not the counts handle's", who); return KGPU_ERR_INVALID_ARG; }
    CountsArgs a{};
    // (the renders' per-sentence scratch holds the launch's per-workgroup totals: one render or count is pending per context)
    if (int rc = records_batch(c, r, (size_t)count_blocks(r.n) * COUNT_PARTIAL_WORDS * 8, nullptr, a.b)) return rc;
    a.w = word_table(k->words);
    a.dense = (unsigned long long *)k->d_dense;
    a.slots = (CountSlot *)k->d_slots; a.slot_mask = (uint32_t)(k->table_slots - 1);
    a.arena = (uint8_t *)k->d_arena; a.arena_bytes = k->key_bytes;
    a.stats = (unsigned long long *)k->d_stats;
    k->version.fetch_add(1, std::memory_order_acq_rel);
    k->sentences.fetch_add(r.n, std::memory_order_relaxed);
    return records_launched(c, launch_count_words(a, c->stream), who, "count", ~0ull);
}

extern "C" int kgpu_count_words_device(kgpu_ctx *c, kgpu_counts *k, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                       const kgpu_token *d_tokens, const uint64_t *d_tok_offsets) {
    const char *who = "kgpu_count_words_device";
    if (!c || !k || !d_offsets || !d_tok_offsets || (n && (!d_utf8 || !d_tokens))) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    if (k->words->dict != c->dict) { set_error("%s: the context's dictionary is not the counts handle's", who); return KGPU_ERR_INVALID_ARG; }
    if (int rc = begin_records_call(c, who)) return rc;
    return enqueue_count(c, k, DeviceRecords{d_utf8, d_offsets, n, d_tokens, d_tok_offsets, nullptr, nullptr}, who);
}

extern "C" int kgpu_ctx_sync_count(kgpu_ctx *c, uint64_t *n_counted) {
    if (!c) { set_error("kgpu_ctx_sync_count: null ctx"); return KGPU_ERR_INVALID_ARG; }
    if (n_counted) *n_counted = 0;
    if (!c->lines_report.pending) return KGPU_OK;
    HIPCHECK(hipSetDevice(c->dict->device));
    uint64_t h[2];   // [0] tokens counted, [1] bit 0: a bad record, bit 1: a token found no room
    if (int rc = c->lines_report.wait(h)) return rc;
    if (n_counted) *n_counted = h[0];
    if (h[1] & 1) {
        set_error("kgpu_ctx_sync_count: a token record names a class, morph id or surface outside the dictionary or its sentence; reset the counts handle");
        return KGPU_ERR_INVALID_ARG;
    }
    if (h[1] & 2) {
        set_error("kgpu_ctx_sync_count: the counts handle's table or key arena is full: tokens were added to overflow_tokens");
        return KGPU_ERR_CAPACITY;
    }
    return KGPU_OK;
}

// ---- the host calls: the lines calls' chunk pipeline with a chunk that returns status bytes only -----------------------------------------------
namespace {

// One count chunk: when its records are final the count kernel reads them and mirrors the status bytes into c's mapped lines_status.
struct CountChunk : RecordsChunk {
    // Wait for the chain (reruns included: the records are final behind it), count, wait for the count.  overflow: a token found no room (the call goes on).
    int finish(kgpu_ctx *c, kgpu_counts *k, uint64_t lo, uint8_t *status, bool &overflow, const char *who) const {
        int rc = kgpu_ctx_sync(c, nullptr);   // (24-byte records with capacity token_bound: never too small)
        if (rc || (rc = enqueue_count(c, k, records(c), who))) return rc;
        rc = kgpu_ctx_sync_count(c, nullptr);
        if (rc == KGPU_ERR_CAPACITY) { overflow = true; rc = KGPU_OK; }
        if (rc) return rc;
        if (status && n) std::memcpy(status + lo, c->lines_status.h, (size_t)n);
        return KGPU_OK;
    }
};

// The body of both host calls, under the handle's shared lock (the caller's, for the whole call).
int count_call(const ChunkSource &src, kgpu_counts *k, uint8_t *status, const char *who) {
    bool overflow = false;
    const int rc = run_chunks(src, CountChunk{}, who, [&](ChunkJob<CountChunk> &j) { return j.out.finish(j.c, k, j.lo, status, overflow, who); });
    if (rc || !overflow) return rc;
    set_error("%s: the counts handle's table or key arena is full: tokens were added to overflow_tokens (everything else is counted)", who);
    return KGPU_ERR_CAPACITY;
}

}  // namespace

extern "C" int kgpu_count_batch(kgpu_counts *k, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint8_t *status) {
    const char *who = "kgpu_count_batch";
    if (!k || !offsets) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    std::shared_lock<std::shared_mutex> g(k->mu);
    ChunkSource src;
    if (int rc = src.packed(k->words->dict, who, utf8, offsets, n, false, false)) return rc;
    return count_call(src, k, status, who);
}

extern "C" int kgpu_count_text(kgpu_counts *k, const uint8_t *text, uint64_t len, uint8_t *status, uint64_t status_capacity, uint64_t *n_lines) {
    const char *who = "kgpu_count_text";
    if (!k || (len && !text) || !n_lines) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    *n_lines = 0;
    std::shared_lock<std::shared_mutex> g(k->mu);
    ChunkSource src;
    if (int rc = src.block(k->words->dict, who, text, len, false)) return rc;
    *n_lines = src.n;
    if (status && src.n > status_capacity) {
        set_error("%s: status capacity %llu, the block has %llu lines (nothing was counted)", who, (unsigned long long)status_capacity, (unsigned long long)src.n);
        return KGPU_ERR_CAPACITY;
    }
    return count_call(src, k, status, who);
}

// ---- the read-out ----------------------------------------------------------------------------------------------------------------------------
extern "C" int kgpu_counts_read(kgpu_counts *k, uint64_t top, uint8_t *words, uint64_t words_capacity, uint64_t *word_offsets, uint64_t *counts,
                                uint64_t entries_capacity, uint64_t *n_entries, uint64_t *n_bytes) {
    const char *who = "kgpu_counts_read";
    if (!k || !n_entries || !n_bytes) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    std::unique_lock<std::shared_mutex> g(k->mu);
    const uint64_t ver = k->version.load(std::memory_order_acquire);
    if (k->cached_version != ver) {   // (the sizing call and the call that fetches share one read-out)
        kgpu_words *w = k->words;
        kgpu_dict *d = w->dict;
        HIPCHECK(hipSetDevice(d->device));
        const size_t nk = (size_t)d->info.n_morphs, rows = nk + (size_t)d->info.n_unk_morphs;
        unsigned long long st[COUNT_STAT_WORDS];
        HIPCHECK(hipMemcpy(st, k->d_stats, sizeof st, hipMemcpyDeviceToHost));
        std::vector<uint64_t> dense(rows);
        if (rows) HIPCHECK(hipMemcpy(dense.data(), k->d_dense, rows * 8, hipMemcpyDeviceToHost));
        std::vector<CountSlot> slots;
        std::vector<uint8_t> arena;
        if (st[1]) {
            slots.resize((size_t)k->table_slots);
            HIPCHECK(hipMemcpy(slots.data(), k->d_slots, slots.size() * sizeof(CountSlot), hipMemcpyDeviceToHost));
            arena.resize((size_t)std::min<uint64_t>(st[0], k->key_bytes));
            if (!arena.empty()) HIPCHECK(hipMemcpy(arena.data(), k->d_arena, arena.size(), hipMemcpyDeviceToHost));
        }
        std::vector<Entry> e;
        bool need_keys = false;
        for (size_t r = 0; r < nk && !need_keys; ++r) need_keys = dense[r] && (w->h_rows[r].len_flags & WORD_SURFACE);
        if (need_keys) dict_key_table(d);
        for (size_t r = 0; r < rows; ++r) {
            if (!dense[r]) continue;
            const WordRow &row = w->h_rows[r];
            if (!(row.len_flags & WORD_SURFACE)) e.push_back(Entry{w->h_names.data() + row.off, row.len_flags & WORD_LEN_MASK, dense[r]});
            else if (r < nk) e.push_back(Entry{d->key_bytes.data() + d->key_off[r], d->key_off[r + 1] - d->key_off[r], dense[r]});
            // (an unknown row whose word is the surface is never counted by its row)
        }
        for (const CountSlot &s : slots) {
            if (!s.tag || !s.count) continue;
            const uint64_t at = ((s.tag & 0xFFFFFFFFull) - 1) * 8;
            if (at + COUNT_ENTRY_HEAD > arena.size()) { set_error("%s: a slot names bytes outside the key arena", who); return KGPU_ERR_INTERNAL; }
            uint32_t len;
            std::memcpy(&len, arena.data() + at, 4);
            if (at + COUNT_ENTRY_HEAD + len > arena.size()) { set_error("%s: a slot names bytes outside the key arena", who); return KGPU_ERR_INTERNAL; }
            e.push_back(Entry{arena.data() + at + COUNT_ENTRY_HEAD, len, s.count});
        }
        merge_and_order(e, 0);
        flatten(e, k->cached_words, k->cached_off, k->cached_counts);
        k->cached_version = ver;
    }
    return deliver(who, k->cached_words, k->cached_off, k->cached_counts, top, words, words_capacity, word_offsets, counts, entries_capacity, n_entries, n_bytes);
}

// Test hook (host only, not in the header): rule 5 without a device.  n_in unmerged entries -- entry i is in_words[in_offsets[i] .. in_offsets[i + 1])
// with in_counts[i] -- -> the merged, ordered, `top`-cut list by the read-out's protocol.
extern "C" int kgpu_debug_counts_order(const uint8_t *in_words, const uint64_t *in_offsets, const uint64_t *in_counts, uint64_t n_in, uint64_t top,
                                       uint8_t *words, uint64_t words_capacity, uint64_t *word_offsets, uint64_t *counts, uint64_t entries_capacity,
                                       uint64_t *n_entries, uint64_t *n_bytes) {
    const char *who = "kgpu_debug_counts_order";
    if (!n_entries || !n_bytes || (n_in && (!in_offsets || !in_counts))) { set_error("%s: null argument", who); return KGPU_ERR_INVALID_ARG; }
    std::vector<Entry> e;
    for (uint64_t i = 0; i < n_in; ++i) {
        if (in_offsets[i + 1] < in_offsets[i] || (in_offsets[i + 1] != in_offsets[i] && !in_words)) { set_error("%s: bad offsets", who); return KGPU_ERR_INVALID_ARG; }
        e.push_back(Entry{in_words + in_offsets[i], in_offsets[i + 1] - in_offsets[i], in_counts[i]});
    }
    merge_and_order(e, 0);
    std::vector<uint8_t> w;
    std::vector<uint64_t> off, cnt;
    flatten(e, w, off, cnt);
    return deliver(who, w, off, cnt, top, words, words_capacity, word_offsets, counts, entries_capacity, n_entries, n_bytes);
}
