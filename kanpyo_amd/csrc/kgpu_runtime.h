// kanpyo_amd/csrc/kgpu_runtime.h -- the host runtime's own types and the functions its files share: kgpu_dict.cpp (dictionary),
// kgpu_ctx.cpp (contexts, launch chain, the shared head and tail of the four record consumers' enqueues), kgpu_host.cpp (large host calls: the chunk frame of the lines, words, encode and count calls), kgpu_small.cpp (small calls), kgpu_multi.cpp (the
// multi-device entry points), kgpu_split_host.cpp (lines of a raw block), kgpu_lattice_call.h (the frame of the kept-lattice calls: DOT documents, N-best, probabilities, modes), kgpu_words_host.cpp (wakati), kgpu_count_host.cpp (word counts), kgpu_encode_host.cpp (vocabulary ids), kgpu_normalize_host.cpp (text normalisation).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdlib>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <vector>

#include "kgpu_chain.h"
#include "kgpu_chunk_policy.h"

#define HIPCHECK(expr)                                                                  \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return KGPU_ERR_HIP;                                                        \
        }                                                                               \
    } while (0)

namespace kgpu {

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return KGPU_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 4 + 256;
        HIPCHECK(hipMalloc(&p, want));
        bytes = want;
        return KGPU_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// Pinned host memory, optionally device-mapped (the device then reads / writes it over PCIe by itself).
struct PinBuf {
    void *h = nullptr, *d = nullptr; size_t bytes = 0;
    int ensure(size_t need, bool mapped) {
        if (need <= bytes) return KGPU_OK;
        release();
        size_t want = need + need / 4 + 4096;
        if (hipHostMalloc(&h, want, mapped ? hipHostMallocMapped : hipHostMallocDefault) != hipSuccess) { h = nullptr; set_error("pinned allocation of %zu bytes failed", want); return KGPU_ERR_HIP; }
        d = h;
        if (mapped && hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipHostFree(h); h = d = nullptr; set_error("hipHostGetDevicePointer failed"); return KGPU_ERR_HIP; }
        bytes = want;
        return KGPU_OK;
    }
    void release() { if (h) (void)hipHostFree(h); h = d = nullptr; bytes = 0; }
};

// A launch that publishes two 64-bit words to the host (the render: [0] bytes, [1] a bad record; the split's carry kernel: [0] lines, [1] packed bytes):
// 16 mapped bytes the kernel stores into, an event behind the launch, and the capacity the launch was given, which the sync compares the words with.
struct HostReport {
    PinBuf ctl;
    hipEvent_t ev = nullptr;
    bool pending = false;
    uint64_t cap = 0;
    // an aligned normalise (kgpu_normalize_host.cpp) publishes two SIZES: word [1] is its edit count, compared with cap1 as word [0] is with cap, and kept
    // in word1 for kgpu_ctx_sync_normalize_aligned; arm() makes the report an ordinary one again
    bool two_sizes = false;
    uint64_t cap1 = 0, word1 = 0;
    const char *bad_what = nullptr;              // what a raised word [1] means when it is not a bad token record (the pack: an input range); arm() clears it
    int arm();                                   // before the launch: a previous use waited out (its words are about to be reset), block and event there, words zero
    unsigned long long *dev() const { return (unsigned long long *)ctl.d; }   // what the launch is given
    int record(hipStream_t stream, uint64_t cap);   // behind the launch
    int wait(uint64_t words[2]);                 // the launch is through: its two words
    void release();                              // (waits for a launch still pending)
};

}  // namespace kgpu

using namespace kgpu;  // (a private header of the runtime's translation units, which all speak this namespace's vocabulary)

struct Combiner;  // kgpu_small.cpp: concurrent small calls sharing a launch

struct kgpu_dict {
    int device = 0;
    Combiner *combiner = nullptr;
    int combiner_callers() const;  // threads inside the small-call entry point right now
    DictView view{};
    kgpu_dict_info info{};
    std::vector<void *> allocs;
    std::mutex pool_mu;
    std::vector<kgpu_ctx *> pool;
    Steering steer;   // the launch chain's dictionary-wide state (kgpu_chain.h)
    // Streams shared by the contexts created without one.  HIP multiplexes streams onto three
    // hardware queues: a 4th stream queues behind the 1st and unbalances them (measured -25 %), so any
    // number of contexts shares three streams; each context waits on its own completion event.  All of them are created with the
    // dictionary's first such context (under pool_mu) and stay until the dictionary goes: a batch reads the vector without the lock.
    // Every batch goes to the least-loaded of them (kgpu_chain.h: pick_stream; kgpu_ctx.cpp: ctx_begin_batch): stream_load[k] is the weight of
    // the batches in flight on streams[k] as the host knows it, stream_batches[k] what it has been given (kgpu_debug_stream_batches: the tests' witness).
    std::vector<hipStream_t> streams;
    std::unique_ptr<std::atomic<uint64_t>[]> stream_load, stream_batches;
    std::atomic<unsigned> stream_cursor{0};
    // A second set for chains that START with the windowed kernel (batches of long sentences: kgpu_ctx.cpp, ctx_pick_stream): such a launch holds a thousand
    // single-wavefront workgroups for milliseconds and its slots empty out one by one, so the chip fills only when more of them overlap than the four launches
    // the pool kernel wants -- one stream per context, up to eight, created when the first such batch arrives (round 5: cfg 5 2.97 -> 3.96 Gchar/s).
    std::vector<hipStream_t> long_streams;
    unsigned next_long = 0;
    std::vector<uint32_t> left_of_rank, right_of_rank;  // device (ranked) context id -> the dictionary's own; empty = identity
    // kgpu_dict_set_features (kgpu_features.cpp): every known and unknown morph's features joined with ',', in the one index space of the
    // morph records (unknown id u at row n_morphs + u - 1): row r is feat[feat_off[r] .. feat_off[r + 1]).  Set once, before any lines call.
    std::mutex feat_mu;
    const uint8_t *feat = nullptr;
    const uint32_t *feat_off = nullptr;
    // ... and the same rows as a graphviz node's label has them ("*" dropped, '/'-joined): built with the pool above, kept on the host, uploaded by the
    // handle's first graphviz call (ensure_label_pool, under feat_mu) -- a handle that draws no lattice spends no HBM on it
    std::vector<uint8_t> label_host;
    std::vector<uint32_t> label_off_host;
    const uint8_t *label = nullptr;
    const uint32_t *label_off = nullptr;
    // ... and a copy of the two blobs themselves, which kgpu_words_create parses again for its per-row word table (host memory: their size)
    std::vector<uint8_t> feat_blob_known, feat_blob_unk;
    // The word counts' read-out resolves a known id to its KEY (kgpu_count_host.cpp: dict_key_table): key id k is key_bytes[key_off[k - 1] .. key_off[k]).
    // Built lazily, once, from the double array as the caller gave it (da_host, dup_host: kept for this and released when the table is there).
    std::mutex keys_mu;
    bool keys_built = false;
    std::vector<DaNode> da_host;
    std::vector<std::pair<int64_t, uint64_t>> dup_host;
    std::vector<uint8_t> key_bytes;
    std::vector<uint64_t> key_off;
    // One reference for the handle the caller holds plus one per live context: the tables and the shared
    // streams go when the last one does (a context outliving kgpu_dict_destroy keeps working).
    // The normaliser's tables (kgpu_normalize_host.cpp: ensure_norm_tables): dictionary-independent, uploaded by the handle's first normalise call
    bool norm_ready = false;   // (under feat_mu)
    NormTables norm{};
    std::atomic<int> refs{1};
    std::atomic<bool> closed{false};   // kgpu_dict_destroy has run: a words handle that outlives it empties the context pool when it goes
};

// A words handle (kgpu_words_host.cpp): a field, a filter and a separator for one dictionary, and the device tables made from them.  Immutable.
struct kgpu_words {
    kgpu_dict *dict = nullptr;          // holds a reference, as a context does
    int32_t field = -1;
    uint32_t filter = 0, sep = ' ';
    void *d_rows = nullptr, *d_names = nullptr;   // WordRow per feature row; the pool of distinct names
    std::vector<WordRow> h_rows;        // ... and their host copies: a counts handle's read-out resolves a row to its bytes
    std::vector<uint8_t> h_names;
    std::atomic<int> refs{1};           // the caller's handle, and one per counts handle made from it: the tables go with the last (words_release)
};

// A counts handle (kgpu_count_host.cpp): the word frequencies of everything added to it, on the device, by a words handle's field and filter.
struct kgpu_counts {
    kgpu_words *words = nullptr;        // holds a reference (its tables and, through it, the dictionary)
    uint64_t table_slots = 0, key_bytes = 0;
    void *d_dense = nullptr, *d_slots = nullptr, *d_arena = nullptr, *d_stats = nullptr;
    std::shared_mutex mu;               // adding calls share it, read-out and reset take it alone
    std::atomic<uint64_t> sentences{0};
    std::atomic<uint64_t> version{1};   // bumped by every add and reset: the merged read-out below is that of `cached_version`
    uint64_t cached_version = 0;
    std::vector<uint8_t> cached_words;
    std::vector<uint64_t> cached_off, cached_counts;
};

// A vocabulary handle (kgpu_encode_host.cpp): a frozen word -> id table on the device, by a words handle's field and filter.  Immutable.
struct kgpu_vocab {
    kgpu_words *words = nullptr;        // holds a reference (its tables and, through it, the dictionary)
    uint32_t flags = 0;
    int32_t unk_id = 0, bos_id = 0, eos_id = 0;
    uint64_t n_words = 0, table_slots = 0, key_bytes = 0, rows_resolved = 0;
    void *d_row_id = nullptr, *d_slots = nullptr, *d_arena = nullptr;
    // a WordPiece handle (kgpu_vocab_create_wordpiece): the continuation table (the initial table's pointers again when the prefix is empty: `cont_shared`),
    // the 8-byte row entries and the pool behind them, uploaded once; d_row_id stays null -- the plain kernels never see such a handle
    bool wordpiece = false, cont_shared = false;
    uint32_t max_word_chars = 0, initial_max = 0, cont_max = 0;
    void *d_cont_slots = nullptr, *d_cont_arena = nullptr, *d_wp_rows = nullptr, *d_piece_ids = nullptr, *d_piece_ends = nullptr;
    kgpu_wordpiece_info wp{};
    // the way back (kgpu_decode_device.cpp): the continuation prefix (none on a plain handle), and the id -> arena entry table -- made with the handle, on
    // the host; the handle's first decode call uploads it (under decode_mu) and drops the host copy.  To its callers the handle stays immutable.
    uint8_t prefix[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t prefix_len = 0;
    mutable std::mutex decode_mu;
    mutable std::vector<uint32_t> h_entry;
    mutable void *d_entry = nullptr;
};

// A user dictionary (kgpu_user_batch.cpp): the table of kgpu_user_table.cpp in ONE device allocation, ids as the dictionary's device matrix numbers them.  Immutable.
struct kgpu_userdict {
    kgpu_dict *dict = nullptr;          // holds a reference, as a words handle does
    void *d_block = nullptr;            // slots | groups | entries | key bytes (null: no entries)
    UserTableView view{};               // ... as the kernels are given them
    kgpu_userdict_info info{};
};

struct kgpu_ctx {
    kgpu_dict *dict = nullptr;
    hipStream_t stream = nullptr;       // the stream of the pending / next batch (one of the dictionary's shared streams unless the caller gave one)
    hipStream_t short_stream = nullptr, long_stream = nullptr;   // what `stream` alternates between (library-owned streams only)
    unsigned short_idx = 0;             // short_stream is dict->streams[short_idx]: chosen anew for every batch (ctx_begin_batch)
    uint64_t load_weight = 0;           // what the pending batch added to dict->stream_load[load_idx] (0: nothing; ctx_retire takes it off)
    unsigned load_idx = 0;
    bool own_stream = false;            // the caller's stream: never switched
    ContextSteering steer;              // the launch chain's state of this context (kgpu_chain.h)
    bool batch_begun = false;           // the next batch's short stream is chosen (ctx_begin_batch: by its first ctx_h2d, or by ctx_pick_stream), until ctx_pick_stream has placed the batch
    bool h2d_queued = false;            // ... and a host-buffer path has queued its H2D copy on `stream` (ctx_h2d alone sets it; ctx_pick_stream orders the batch behind it if it goes to a long stream)
    hipEvent_t switch_ev = nullptr;     // orders a batch behind what was queued on the stream the context used before
    hipEvent_t done_ev = nullptr;  // recorded behind the batch's last kernel: contexts may share a stream
    Control *d_ctl = nullptr;
    Control *h_ctl = nullptr;  // pinned + device-mapped: the scan kernel publishes the launch's Control block here
    Control *h_ctl_dev = nullptr;  // device-side address of h_ctl
    bool ctl_dirty = true;     // d_ctl must be zeroed by the host (first launch, or after a failed enqueue)
    uint32_t launch_seq = 0;
    Batch batch{};             // what the pending batch's chain was built from (a rerun builds it again)
    Chain chain;               // the pending launches
    bool tail_pass = false;    // ... are the tail of the batch's chain alone (it had been left out and a sentence needed it)
    Chain first_pass;          // ... then the chain that ran first
    Control tail_saved{};      // ... what it had published (the length of the list the tail serves is copied back from here: lives in the context)
    uint32_t event_every = 1;  // KGPU_PROFILE_SAMPLED: HIP events on every 4th launch only
    DevBuf arena, stage, tok_count;
    size_t arena_initial = 0;  // the arena's first size on the tokenize path: ARENA_INITIAL, or KGPU_ARENA_INITIAL as the context found it when it was created
    // host-buffer path staging
    DevBuf in_utf8, in_off, out_tok, out_off, out_status;
    PinBuf pin_in, pin_out;       // large host calls: input staging (offsets | bytes), mapped result block (records | first | token offsets | status)
    DevBuf in_block;              // ... and the device copy of the input block
    // single-launch small calls: one pinned, device-mapped block (input | offsets | tokens | token offsets | status)
    uint8_t *sm_host = nullptr, *sm_dev = nullptr;
    uint32_t sm_seq = 0;
    // the CLI's output lines (kgpu_format.hip): per-sentence scratch, what the render's scan publishes ([0] bytes, [1] a bad record), and for a chunk
    // of the host lines calls (LinesChunk) the mapped text, text offsets and status (the render's stores are the transfer)
    DevBuf lines_len;
    HostReport lines_report;
    PinBuf lines_text, lines_off, lines_status;
    // a chunk of a kept-lattice call (kgpu_lattice_call.h; graphviz, N-best, marginals / samples, mode, user dictionary): the lattice descriptors (LAT_DESC_WORDS per sentence),
    // the 8-byte words of the call's per-chunk arrays (what its scans run over: LatticeOps::chunk_words), and the block its write launch fills
    DevBuf lat_desc, lat_words, lat_out;
    // read_line + trim_end on the device (kgpu_split.hip): the tile aggregates, what the carry kernel publishes ([0] lines, [1] packed bytes), and
    // for kgpu_tokenize_text_lines the device copy of the raw block, its packed lines and their offsets
    DevBuf split_agg, split_raw, split_text, split_off;
    HostReport split_report;
    // text normalisation (kgpu_normalize.hip): the host forms' normalised text on the device (their offsets and status bytes: out_off, out_status)
    DevBuf norm_text;
    // ... and of the aligned forms and kgpu_source_spans_batch: edit records, their offsets, spans
    DevBuf norm_edits, norm_eoff, span_out;
    // last enqueued batch (for the arena-overflow retry and for sync)
    BatchArgs last{};
    bool pending = false;
    LaunchPlan plan{};
    int aux_form = 0;    // what the last batch's scan + compaction was (launch_scan_compact; kgpu_debug_aux_form)
    int aux_mode = -1;   // KGPU_AUX_LAUNCH as the context found it when it was created (launch_scan_compact; -1: the chain decides)
    DevBuf ovf;
    DevBuf stat_slots;                             // profiling runs: per-wavefront counters of the pool kernel (BatchArgs::stat_slots)
    std::vector<unsigned long long> stat_host;
    // profiling
    bool profiling = false;   // KGPU_PROFILE_EVENTS
    bool count_work = false;  // KGPU_PROFILE_WORK
    bool count_no_t = false;  // KGPU_PROFILE_NO_T
    uint32_t stop_after = 0;  // kgpu_ctx_set_ablation: measurement mode, 0 = off
    kgpu_work work{};
    uint64_t phase[10] = {0};
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    kgpu_profile prof{};
    kgpu_routing rt{};
};


#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace kgpu {

// Host side of the 8-byte records (include/kanpyo_gpu.h, kgpu_token8): n sentences' records -> 24-byte kgpu_token, position / start as running sums per
// sentence.  stream: the 24-byte records go out with non-temporal stores (three 8-byte movnti per token; `out` 8-byte aligned) -- the expansion of a large
// call writes hundreds of megabytes nobody reads back soon, and an ordinary store first READS every line it is about to overwrite: a third of the
// expansion's memory traffic, and the expansion is a memory-bandwidth job.  The caller fences (expand_fence) before it publishes the result.
inline void expand_tokens(const kgpu_token8 *in, const uint64_t *tok_offsets, const uint32_t *first, uint64_t n, kgpu_token *out, bool stream) {
    const uint64_t base = tok_offsets[0];
#if defined(__x86_64__)
    if (stream && ((uintptr_t)out & 7u) == 0) {
        for (uint64_t s = 0; s < n; ++s) {
            uint32_t pos = first[2 * s], st = first[2 * s + 1];
            for (uint64_t k = tok_offsets[s] - base, e = tok_offsets[s + 1] - base; k < e; ++k) {
                const uint32_t p = in[k].packed, chars = KGPU_T8_CHARS(p), bytes = KGPU_T8_BYTES(p);
                long long *o = (long long *)(out + k);
                _mm_stream_si64(o, (long long)((uint64_t)(uint32_t)in[k].id | ((uint64_t)KGPU_T8_CLS(p) << 32)));
                _mm_stream_si64(o + 1, (long long)((uint64_t)pos | ((uint64_t)st << 32)));
                _mm_stream_si64(o + 2, (long long)((uint64_t)(st + chars) | ((uint64_t)bytes << 32)));
                pos += bytes; st += chars;
            }
        }
        return;
    }
#endif
    for (uint64_t s = 0; s < n; ++s) {
        uint32_t pos = first[2 * s], st = first[2 * s + 1];
        for (uint64_t k = tok_offsets[s] - base, e = tok_offsets[s + 1] - base; k < e; ++k) {
            const uint32_t p = in[k].packed, chars = KGPU_T8_CHARS(p), bytes = KGPU_T8_BYTES(p);
            out[k] = kgpu_token{in[k].id, KGPU_T8_CLS(p), pos, st, st + chars, bytes};
            pos += bytes; st += chars;
        }
    }
}
inline void expand_fence() {
#if defined(__x86_64__)
    _mm_sfence();
#endif
}
constexpr uint64_t EXPAND_STREAM_MIN_TOKENS = 32768;   // from this many tokens (768 KB of records) in one chunk on: non-temporal stores
inline bool expand_stream_wanted(uint64_t tokens) {       // (KGPU_EXPAND_STREAM=0 / 1: measurement, forces ordinary / non-temporal stores)
    static const int mode = [] { const char *e = getenv("KGPU_EXPAND_STREAM"); return e ? atoi(e) : -1; }();
    return mode >= 0 ? mode != 0 : tokens >= EXPAND_STREAM_MIN_TOKENS;
}

struct WorkerPool {
    std::mutex mu; std::condition_variable cv; std::deque<std::function<void()>> q; std::vector<std::thread> th;
    std::mutex done_mu; std::condition_variable done_cv;
    unsigned start();                         // threads running (0: none could be created)
    void submit(std::function<void()> f);
    void wait_zero(std::atomic<int> &counter); // until the tasks counted there are through
    void task_done(std::atomic<int> &counter); // a task's last statement
};
WorkerPool &workers();
// The hooks of the kept-lattice calls (kgpu_lattice_call.h), one slot per family: KGPU_HOST_<NAME>_CHUNK_SENTS, sentences per chunk (0: the default), and
// KGPU_HOST_<NAME>_ARENA_INITIAL / _ARENA_MAX, the bytes of the scratch arena a chunk's kept lattices may use at first / at most (0: the whole arena /
// ARENA_MAX): tests of the overflow protocol.  LATTICE_HOOK_NAMES (kgpu_dict.cpp) holds the <NAME>s in this order.
enum LatticeHook : uint32_t { HOOK_GRAPHVIZ, HOOK_NBEST, HOOK_PROB, HOOK_MODE, HOOK_USER, LATTICE_HOOKS };
struct LatticeHooks { uint64_t chunk_sents = 0, arena_initial = 0, arena_max = 0; };
struct TestHooks { bool no_small_calls = false, plain_leaves = false, byte_trie = false; uint64_t chunk_bytes = 4ull << 20, chunk_sents = 16384, depth = 12, multi_chunk_sents = 0, arena_initial = 0; int aux_launch = -1; LatticeHooks lattice[LATTICE_HOOKS]; };
TestHooks test_hooks();  // test-only environment hooks, read once per process (or per call under KGPU_TEST_HOOKS_REREAD)
bool env_flag_now(const char *name);

// kgpu_dict.cpp
unsigned planned_streams();        // shared streams per dictionary (by the hardware queues the process has)
unsigned planned_long_streams();   // ... and streams for chains that start with the windowed kernel
void dict_release(kgpu_dict *d);   // one reference less: the last one frees the dictionary

// kgpu_ctx.cpp
constexpr size_t ARENA_INITIAL = 1ull << 28;  // 256 MiB; only the general (HBM-scratch) kernel uses it, grows x2 on demand
constexpr size_t ARENA_MAX = 1ull << 37;      // 128 GiB
// the pooled contexts of a dictionary (one per call in flight)
int pool_get(kgpu_dict *d, kgpu_ctx **c);
void pool_put(kgpu_dict *d, kgpu_ctx *c);   // (it goes back without a batch begun: a path that queued copies with ctx_h2d and waited for them itself, no tokenize batch behind them, left the flags set)
// A pooled context for the length of a scope: `rc` is pool_get's answer, and however the scope is left the context goes back.  put(): back before the scope ends.
struct PooledCtx {
    kgpu_dict *d = nullptr; kgpu_ctx *c = nullptr; int rc = KGPU_OK;
    PooledCtx() = default;                                  // (empty: get() leases later)
    explicit PooledCtx(kgpu_dict *d_) { get(d_); }
    PooledCtx(const PooledCtx &) = delete; PooledCtx &operator=(const PooledCtx &) = delete;
    ~PooledCtx() { put(); }
    int get(kgpu_dict *d_) { d = d_; return rc = pool_get(d, &c); }
    void put() { if (c) { pool_put(d, c); c = nullptr; } }
};
int ctx_h2d(kgpu_ctx *c, void *dst, const void *src, size_t bytes, const char *what);   // a batch's H2D copy: begins the batch (its stream is chosen), then the copy on c->stream
int tokenize_device_impl(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                         kgpu_token *d_tokens, kgpu_token8 *d_tokens8, uint32_t *d_first, uint8_t *status8, uint64_t *toff8, uint64_t token_capacity,
                         uint64_t *d_tok_offsets, uint8_t *d_status, const char *who);
// A batch's records where they lie in device memory, with the optional mirror of its status bytes (status_out: mapped host memory): what the
// four consumers below are given.  Each runs on c->stream behind whatever is queued there, with the context's lines_report and lines_len: one is pending per context.
struct DeviceRecords {
    const uint8_t *d_utf8; const uint64_t *d_offsets; uint64_t n; const kgpu_token *d_tokens; const uint64_t *d_tok_offsets;
    const uint8_t *status_in; uint8_t *status_out;
};
// The device entry points' shared preamble: the context's tokenize batch is synced, its device is current, a pending report is waited for (KGPU_ERR_CAPACITY passes).
int begin_records_call(kgpu_ctx *c, const char *who);
// An enqueue's head: the report armed, lines_len of scratch_bytes at least, `b` filled from r and the context (unit_offsets: RecordsBatch::text_offsets) ...
int records_batch(kgpu_ctx *c, const DeviceRecords &r, size_t scratch_bytes, uint64_t *d_unit_offsets, RecordsBatch &b);
// ... and its tail: a launch error (hipError_t) becomes "<who>: <what> launch: ..."; else the report is recorded with the capacity the sync compares with
int records_launched(kgpu_ctx *c, int launch_error, const char *who, const char *what, uint64_t capacity);
WordTable word_table(const kgpu_words *w);   // kgpu_words_host.cpp
int enqueue_lines(kgpu_ctx *c, const DeviceRecords &r, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, const char *who);
// ... its wakati lines (kgpu_words_host.cpp over kgpu_words.hip); waited for by kgpu_ctx_sync_lines as well
int enqueue_words(kgpu_ctx *c, const kgpu_words *w, const DeviceRecords &r, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, const char *who);
// kgpu_features.cpp: the per-row entries (known rows, then unknown rows) and the pool of distinct names of a checked spec, from the two blobs
int build_word_table(const uint8_t *known, size_t known_len, const uint8_t *unk, size_t unk_len, uint64_t n_morphs, uint64_t n_unk,
                     const kgpu_words_spec &spec, std::vector<WordRow> &rows, std::vector<uint8_t> &names);

// kgpu_words_host.cpp
void words_release(kgpu_words *w);   // one reference less: the last one frees the tables and lets go of the dictionary
// kgpu_encode_host.cpp: the vocabulary ids of a batch's records on c->stream (waited for by kgpu_ctx_sync_lines, which reports the ids); width 0: ragged
// spans (may be null): the span instantiation of the write kernel, a span and a token index beside every id (kgpu_encode_device_spans)
int enqueue_encode(kgpu_ctx *c, const kgpu_vocab *v, const DeviceRecords &r, int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id, uint64_t *d_id_offsets, const char *who,
                   const SpanOut *spans = nullptr);
void dict_key_table(kgpu_dict *d);   // kgpu_count_host.cpp: the dictionary's id -> key table (d->key_bytes, d->key_off), built by the first caller that needs it
// kgpu_count_host.cpp: the count of a batch's records on c->stream behind whatever is queued there (waited for by kgpu_ctx_sync_count)
int enqueue_count(kgpu_ctx *c, kgpu_counts *k, const DeviceRecords &r, const char *who);

// kgpu_normalize_host.cpp: the normalisation of a batch in device memory on c->stream behind whatever is queued there (waited for by kgpu_ctx_sync_normalize)
int enqueue_normalize(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint8_t *d_text, uint64_t text_capacity,
                      uint64_t *d_text_offsets, uint8_t *d_status, const char *who);
// ... with the lines' edit records (waited for by kgpu_ctx_sync_normalize_aligned)
int enqueue_normalize_aligned(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint8_t *d_text, uint64_t text_capacity,
                              uint64_t *d_text_offsets, uint8_t *d_status, kgpu_norm_edit *d_edits, uint64_t edit_capacity, uint64_t *d_edit_offsets, const char *who);

int require_features(kgpu_dict *d, const char *who);   // KGPU_ERR_INVALID_ARG unless kgpu_dict_set_features has been called
int ensure_label_pool(kgpu_dict *d);                   // kgpu_features.cpp: the graphviz label pool on the device (first call uploads it)

// kgpu_host.cpp
void parallel_copy(void *dst, const void *src, size_t bytes);
bool is_pinned_host(const void *p);
int batch_depth();                                                               // the ring of the host batch calls
bool batch_is_pinned(const uint8_t *utf8, const uint64_t *offsets, uint64_t n);  // ... whose input is copied from directly when it is pinned
int check_host_batch(const char *who, const uint64_t *offsets, uint64_t n, const uint8_t *utf8);   // a host batch's offsets are monotone, its bytes are there
// The records a batch of n sentences / `total` bytes can produce: tokens <= chars + 1 <= bytes + 1 per sentence, so a buffer of this many is never too small.
inline uint64_t token_bound(uint64_t total, uint64_t n) { return total + n + 1; }
// A finished chunk's results in host memory: 8-byte records, (position, start) of every sentence's first token, token offsets, status bytes.
struct MergeSrc { const kgpu_token8 *rec; const uint32_t *first; const uint64_t *toff; const uint8_t *st; };
// The input of one chunk of a host call on a pooled context: it goes to the device as ONE block [offsets | bytes] (c->in_block, staged in c->pin_in
// unless it is copied from pinned memory directly).  The offsets are as the caller has them: the kernels subtract offsets[0], the text pointer is biased by it.
struct ChunkInput {
    uint64_t n = 0, total = 0;                             // sentences, bytes
    size_t in_off = 0;                                     // the offsets' share of the block: the bytes follow
    int prepare(kgpu_ctx *c, uint64_t n, uint64_t total, bool staged);   // the layout, and c's buffers big enough for it
    const uint64_t *d_offsets(const kgpu_ctx *c) const { return (const uint64_t *)c->in_block.p; }
    const uint8_t *d_text(const kgpu_ctx *c, uint64_t base) const { return (const uint8_t *)c->in_block.p + in_off - base; }   // (offsets start at `base`)
};
int upload_input(kgpu_ctx *c, const ChunkInput &in, const uint8_t *utf8, const uint64_t *off, bool pinned_in);   // kgpu_host.cpp: the chunk's block to the device (off: its first offset)
// kgpu_split_host.cpp: a raw block of host memory on the splitting context sc: one copy to the device, the split; -> the lines' offsets on the host (sc->split_text /
// sc->split_off hold the packed lines and their offsets on the device until sc is given back)
int split_block(kgpu_ctx *sc, const uint8_t *text, uint64_t len, const char *who, std::vector<uint64_t> &off, uint64_t &lines);
// One chunk of kgpu_tokenize_batch / kgpu_tokenize_batch_multi (kgpu_host.cpp: pipe_submit; kgpu_multi.cpp: shard_submit): its input block, and the
// mapped block c->pin_out the compaction kernel writes the results into: 8-byte records | first | token offsets | status.
struct ChunkBlock {
    ChunkInput in;
    uint64_t cap = 0;                                      // token capacity
    size_t off_first = 0, off_toff = 0, off_status = 0;    // inside pin_out
    int prepare(kgpu_ctx *c, uint64_t n, uint64_t total, bool staged);
    int launch(kgpu_ctx *c, uint64_t base, const char *who) const;        // the chain over the input block, records into pin_out
    MergeSrc results(const kgpu_ctx *c) const;                           // where the host reads them once the chunk is synced
};
// Where the chunks of a lines call deliver: the caller's buffers, what has been delivered so far, and whether a buffer has overflowed (from then on the
// chunks are only counted).  status_after_overflow: the status bytes go out all the same (a status array of n entries whatever happens); not so where
// the status array is bounded by the capacity that overflowed.
struct LinesSink {
    uint8_t *text; uint64_t text_capacity; uint64_t *text_offsets; uint8_t *status;
    bool status_after_overflow;
    uint64_t text_done = 0;
    bool overflow = false;
    uint64_t unit = 1;   // bytes per element of `text`: 1, or 4 where the chunks deliver vocabulary ids (capacities, text_done and the offsets count elements)
};
// What the chunks of a lines call render their records into: the `kanpyo tokenize` lines, a words handle's wakati lines or a vocabulary handle's ids.
// The one value kgpu_tokenize_*_lines, kgpu_tokenize_*_words and kgpu_encode_* differ in, and the one place that tells the three apart (kgpu_host.cpp).
struct Renderer {
    enum Kind { LINES, WORDS, IDS } kind = LINES;
    const kgpu_words *words = nullptr;                     // WORDS
    const kgpu_vocab *vocab = nullptr;                     // IDS
    Renderer() = default;
    explicit Renderer(const kgpu_words *w) : kind(WORDS), words(w) {}
    explicit Renderer(const kgpu_vocab *v) : kind(IDS), vocab(v) {}
    uint64_t unit() const { return kind == IDS ? 4 : 1; }                  // bytes per element of the output (LinesSink::unit)
    const char *noun() const { return kind == IDS ? "id" : "text"; }       // ... and what the overflow message calls it
    size_t first_bytes(uint64_t total, uint64_t n) const;                   // a chunk's output block to begin with (LinesChunk::finish grows it)
    int enqueue(kgpu_ctx *c, const DeviceRecords &r, void *d_out, size_t out_bytes, uint64_t *d_offsets, const char *who) const;
};
// One chunk of a chunked host call on a pooled context, whatever put its input on the device (ChunkSource::stage): the launch chain writes 24-byte
// records that stay in HBM (c->out_tok), and whatever reads them mirrors the status bytes into c's mapped lines_status.
struct RecordsChunk {
    uint64_t n = 0, total = 0;                             // sentences, bytes
    const uint8_t *d_utf8 = nullptr;                       // the chunk's input in device memory (ChunkSource::stage)
    const uint64_t *d_offsets = nullptr;
    int prepare(kgpu_ctx *c, uint64_t n, uint64_t total);                 // c's buffers big enough
    int launch(kgpu_ctx *c, const char *who) const;                       // the chain
    DeviceRecords records(const kgpu_ctx *c) const;                       // what a consumer of the chunk's records is given
};
// ... of a lines, words or encode call: the render behind the chain writes the chunk's text (or ids), chunk-relative offsets and status into c's mapped lines_* blocks.
struct LinesChunk : RecordsChunk {
    Renderer renderer;
    int prepare(kgpu_ctx *c, uint64_t n, uint64_t total);
    int launch(kgpu_ctx *c, const char *who) const;                       // the chain, then the render
    int render(kgpu_ctx *c, const char *who) const;                       // the render of the chunk's records alone
    int finish(kgpu_ctx *c, uint64_t lo, LinesSink &sink, const char *who) const;   // wait, and deliver behind what the sink holds: sentences [lo, lo + n) of the call
};
// Where the lines of a chunked host call come from.  packed(): a packed batch in host memory, each chunk uploaded as one block (ChunkInput) on the batch
// calls' ring; block(): a raw block, copied and split once on a context of its own, which owns the packed lines until the source goes -- a chunk's input
// is a pair of pointers into them.  Both check their input, then the features if asked to, and make the dictionary's device current.
struct ChunkSource {
    kgpu_dict *d = nullptr;
    const uint64_t *offsets = nullptr;                     // host memory, n + 1 entries: what cuts the chunks
    uint64_t n = 0;
    int depth = 0, held_back = 0;                          // the ring (run_pipeline)
    bool empty_chunk = false;
    int packed(kgpu_dict *d, const char *who, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, bool features, bool empty_chunk);   // kgpu_host.cpp
    int block(kgpu_dict *d, const char *who, const uint8_t *text, uint64_t len, bool features);                                             // kgpu_split_host.cpp
    int stage(kgpu_ctx *c, uint64_t lo, uint64_t m, const uint8_t *&d_utf8, const uint64_t *&d_offsets) const;   // sentences [lo, lo + m) on c's stream -> where they lie
    const uint8_t *utf8 = nullptr;                         // packed
    bool pinned = false;
    PooledCtx split;                                       // block: the splitting context ...
    std::vector<uint64_t> split_off;                       // ... and the lines' offsets on the host
};

// kgpu_host.cpp: the packed and the text column of the lines / words / encode host calls, one body over a source and a renderer behind both (`text` holds
// r.unit()-byte elements; the capacity, *n_bytes and the offsets count them)
int batch_lines(kgpu_dict *d, const Renderer &r, const char *who, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);
int text_lines(kgpu_dict *d, const Renderer &r, const char *who, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
               uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes);

// The chunks of a large host call: at most `bytes` / `sents` each (test_hooks() may lower them).
struct ChunkLimits { uint64_t bytes, sents; };
ChunkLimits chunk_limits(uint64_t n);
constexpr int MAX_PIPE_DEPTH = 16;
// A large call goes through in chunks on pooled contexts, several in flight: while chunk k's results are delivered on the host (its records
// expanded, or its text copied), the next chunks compute and the one after them has its input on its way.  `offsets` (n + 1 entries, host memory) cuts the
// chunks; Job has `c`, `lo`, `m` (context, sentences [lo, lo + m)) and whatever submit / finish keep per chunk.  `depth` jobs form the ring, of which
// `held_back` stay out of the device pipeline (their results are still being delivered by the workers).  `finish` delivers the oldest chunk: results
// arrive in order, so the caller's output stays dense.  empty_chunk: a call without sentences still submits one chunk.  host_tasks: what the finishes
// handed to the workers (null: nothing), waited for before the contexts go back to the pool.
template <class Job, class Submit, class Finish>
int run_pipeline(kgpu_dict *d, const uint64_t *offsets, uint64_t n, int depth, int held_back, bool empty_chunk, std::atomic<int> *host_tasks, Submit submit, Finish finish) {
    workers().start();   // (none to be had: the workers' tasks run on this thread)
    const ChunkLimits lim = chunk_limits(n);
    Job jobs[MAX_PIPE_DEPTH];
    int rc = KGPU_OK;
    uint64_t done = 0;
    int head = 0, inflight = 0;  // jobs[head .. head + inflight) (mod depth) are active, oldest first
    while (!rc && (done < n || empty_chunk)) {
        empty_chunk = false;
        if (inflight == depth - held_back) {
            rc = finish(jobs[head]);
            head = (head + 1) % depth; --inflight;
            if (rc) break;
        }
        Job &j = jobs[(head + inflight) % depth];
        if (!j.c && (rc = pool_get(d, &j.c))) break;
        const uint64_t m = cut_chunk(offsets, done, n, lim.sents, lim.bytes);
        j.lo = done; j.m = m;
        if ((rc = submit(j))) {   // (a batch may be queued without what follows it: the context goes back to the pool idle)
            if (j.c->pending) (void)kgpu_ctx_sync(j.c, nullptr);
            break;
        }
        ++inflight;
        done += m;
    }
    while (inflight) {  // drain in order (also after an error: the contexts go back to the pool idle)
        const int r2 = finish(jobs[head]);
        if (!rc) rc = r2;
        head = (head + 1) % depth; --inflight;
    }
    if (host_tasks) workers().wait_zero(*host_tasks);
    for (int k = 0; k < depth; ++k)
        if (jobs[k].c) pool_put(d, jobs[k].c);
    return rc;
}
// The ring over a source's chunks: a copy of `proto` per job; submit is stage, prepare, launch (a context's buffers are then first allocated in the order
// input block, records, mapped blocks: with the records first kgpu_encode_batch measured 2.6 % slower, profiles/experiments/host_frame.txt); finish(job) delivers.
template <class Chunk> struct ChunkJob { kgpu_ctx *c = nullptr; uint64_t lo = 0, m = 0; Chunk out; };
template <class Chunk, class Finish>
int run_chunks(const ChunkSource &src, const Chunk &proto, const char *who, Finish finish) {
    return run_pipeline<ChunkJob<Chunk>>(src.d, src.offsets, src.n, src.depth, src.held_back, src.empty_chunk, nullptr,
        [&](ChunkJob<Chunk> &j) {
            j.out = proto;
            int r;
            if ((r = src.stage(j.c, j.lo, j.m, j.out.d_utf8, j.out.d_offsets)) || (r = j.out.prepare(j.c, j.m, src.offsets[j.lo + j.m] - src.offsets[j.lo]))) return r;
            return j.out.launch(j.c, who);
        },
        finish);
}

// kgpu_small.cpp
Combiner *combiner_new();
void combiner_delete(Combiner *c);
// a call of at most 128 sentences / 16 KB as one launch, shared with concurrent callers: KGPU_OK / KGPU_ERR_CAPACITY served, -1 take the general path
int tokenize_small(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, kgpu_token *tokens, uint64_t token_capacity,
                   uint64_t *tok_offsets, uint8_t *status, uint64_t *n_tokens);
bool small_trace_on();                 // KGPU_SMALL_TRACE
uint64_t cpu_ns();                     // this thread's CPU time
extern std::atomic<uint64_t> g_sc[16];  // ... summed per phase (kgpu_debug_small_cpu; [11]: kgpu_tokenize_batch's hipSetDevice)

}  // namespace kgpu
