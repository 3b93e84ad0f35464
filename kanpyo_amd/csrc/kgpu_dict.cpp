// kanpyo_amd/csrc/kgpu_dict.cpp -- the dictionary handle of include/kanpyo_gpu.h.
//
// Owns: the error string, blob parsing + validation (the panics of the reference's hot path are turned into KGPU_ERR_BAD_DICT at
// create time), the frequency ranking of the context ids, the one-time upload to HBM, the char-trie decision, the test hooks, and
// the load-time hardware-queue set-up with the stream planning that follows from it.  There is NO CPU fallback: without a HIP
// device every entry point that would compute returns KGPU_ERR_NO_DEVICE.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <mutex>
#include <string>
#include <unistd.h>
#include <vector>

#include "kgpu_runtime.h"

namespace kgpu {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

}  // namespace kgpu

using namespace kgpu;

namespace {

struct Reader {
    const uint8_t *p; size_t n, at = 0; bool bad = false;
    Reader(const uint8_t *p_, size_t n_) : p(p_), n(n_) {}
    template <class T> T get() {
        T v{};
        if (at + sizeof(T) > n) { bad = true; return v; }
        std::memcpy(&v, p + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    size_t left() const { return n - at; }
};


}  // namespace

// Test-only environment hooks.  getenv is not thread-safe against setenv, and kgpu_tokenize_batch may be called from many
// threads: the hooks are read under a mutex, ONCE per process -- unless KGPU_TEST_HOOKS_REREAD is set (tests/conftest.py sets
// it: the tests flip the hooks between calls).
bool kgpu::env_flag_now(const char *name) { const char *e = getenv(name); return e && *e && *e != '0'; }
TestHooks kgpu::test_hooks() {
    static std::mutex mu;
    static TestHooks cur;
    static bool init = false;
    std::lock_guard<std::mutex> g(mu);
    if (!init || env_flag_now("KGPU_TEST_HOOKS_REREAD")) {
        init = true;
        cur = TestHooks{};
        cur.no_small_calls = env_flag_now("KGPU_NO_SMALL_CALLS");
        cur.plain_leaves = env_flag_now("KGPU_PLAIN_LEAVES");
        cur.byte_trie = env_flag_now("KGPU_BYTE_TRIE");  // no character-level copy of the trie: every kernel walks the bytes
        if (const char *e = getenv("KGPU_HOST_DEPTH")) cur.depth = strtoull(e, nullptr, 10);
        if (const char *e = getenv("KGPU_HOST_CHUNK_BYTES")) cur.chunk_bytes = strtoull(e, nullptr, 10);
        if (const char *e = getenv("KGPU_HOST_CHUNK_SENTS")) cur.chunk_sents = strtoull(e, nullptr, 10);
        // ... and the three hooks of each kept-lattice family (kgpu_runtime.h: LatticeHooks)
        static const char *const LATTICE_HOOK_NAMES[LATTICE_HOOKS] = {"GRAPHVIZ", "NBEST", "PROB", "MODE", "USER"};
        for (uint32_t h = 0; h < LATTICE_HOOKS; ++h) {
            uint64_t *const field[3] = {&cur.lattice[h].chunk_sents, &cur.lattice[h].arena_initial, &cur.lattice[h].arena_max};
            static const char *const FIELD_NAMES[3] = {"CHUNK_SENTS", "ARENA_INITIAL", "ARENA_MAX"};
            for (int f = 0; f < 3; ++f)
                if (const char *e = getenv((std::string("KGPU_HOST_") + LATTICE_HOOK_NAMES[h] + "_" + FIELD_NAMES[f]).c_str())) *field[f] = strtoull(e, nullptr, 10);
        }
        // ... the first size of a context's scratch arena on the tokenize path, in bytes (0: ARENA_INITIAL; clamped to [1 MiB, ARENA_INITIAL]; read when a context is
        // created): tests of the windowed and the general kernel's overflow protocol (kgpu_ctx_sync doubles the arena and reruns the batch)
        if (const char *e = getenv("KGPU_ARENA_INITIAL")) cur.arena_initial = strtoull(e, nullptr, 10);
        if (const char *e = getenv("KGPU_AUX_LAUNCH")) cur.aux_launch = atoi(e);   // scan + compaction behind a chain: 0 two launches, 1 one, 2 two with the single-wavefront scan (read when a context is created)
        if (const char *e = getenv("KGPU_MULTI_CHUNK_SENTS")) cur.multi_chunk_sents = strtoull(e, nullptr, 10);  // kgpu_tokenize_batch_multi: sentences per device and chunk (tests: many small super-chunks)
    }
    return cur;
}

// Every slot of a double array has ONE parent (its check), so the child edges can only loop back through the root: a root that is itself some
// node's child means a corrupt array whose breadth-first re-indexing (kgpu_chartrie.cpp) would never end.  Such a dictionary is walked byte by byte
// (a walk is bounded by the sentence, whatever the array looks like).
static bool char_trie_buildable(const std::vector<DaNode> &da) {
    if (da.size() < 2) return false;
    const int64_t p = da[1].check;
    if (p < 1 || (size_t)p >= da.size() || p == 1) return true;
    const int64_t b = da[(size_t)p].base, c = 1 - b;
    return !(b >= 0 && c >= 0 && c <= 255);
}
// Test hook (tests/test_chartrie_cpu.py): would kgpu_dict_create build the character-level copy for this index.dict blob?
extern "C" int kgpu_debug_char_trie_usable(const uint8_t *index_blob, size_t blob_len) {
    if (!index_blob || blob_len < 8) return -1;
    uint64_t n = 0;
    std::memcpy(&n, index_blob, 8);
    if (n > (blob_len - 8) / 8) return -1;
    std::vector<DaNode> da((size_t)n);
    if (n) std::memcpy(da.data(), index_blob + 8, (size_t)n * 8);
    CharTrie ct;
    return char_trie_buildable(da) && build_char_trie(da, nullptr, 0, ct) ? 1 : 0;
}

void kgpu::dict_release(kgpu_dict *d) {
    if (d->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    combiner_delete(d->combiner);
    (void)hipSetDevice(d->device);
    for (hipStream_t st : d->streams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipStream_t st : d->long_streams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (void *p : d->allocs) (void)hipFree(p);
    delete d;
}

extern "C" const char *kgpu_last_error(void) { return g_err; }

// Concurrent launches need hardware queues: HIP gives a process GPU_MAX_HW_QUEUES of them (default 4, of which its streams get three), and
// four launches side by side are the optimum of this library.  The variable is read when the HIP runtime initialises, so the
// library sets it itself when it is loaded early enough -- before any HIP / HSA call of the process, i.e. while /dev/kfd is not open yet --
// and the caller has not set it.  Loaded too late (or with the variable set below 5) it runs on three streams and says so
// (kgpu_plan_info.streams, and a warning in kgpu_last_error after kgpu_dict_create).
static bool g_queues_ok = false;
static int g_queues = 4;   // hardware queues the HIP runtime of this process has (or will have): HIP's default unless the variable says otherwise
#ifndef KGPU_HW_QUEUES
#define KGPU_HW_QUEUES 16
#define KGPU_HW_QUEUES_STR "16"
#endif
static bool kfd_is_open() {   // has this process opened the compute driver already (= has a HIP / HSA runtime been initialised)?
    DIR *dir = opendir("/proc/self/fd");
    if (!dir) return true;     // cannot tell: assume the worst (three streams) rather than count on queues that may not be there
    bool found = false;
    char link[300], target[256];
    while (const dirent *e = readdir(dir)) {
        if (e->d_name[0] == '.') continue;
        snprintf(link, sizeof link, "/proc/self/fd/%s", e->d_name);
        const ssize_t k = readlink(link, target, sizeof target - 1);
        if (k > 0) { target[k] = 0; if (strcmp(target, "/dev/kfd") == 0) { found = true; break; } }
    }
    closedir(dir);
    return found;
}
__attribute__((constructor)) static void kgpu_preinit() {
    if (const char *off = getenv("KGPU_NO_PREINIT")) if (*off && *off != '0') return;   // the host does not want its environment touched at load time: three streams unless it sets the variable itself
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    if (e) { g_queues_ok = atoi(e) >= 5; g_queues = std::max(1, atoi(e)); return; }   // the caller's choice stands
    if (kfd_is_open()) return;                          // the runtime is up already: too late, three streams
    setenv("GPU_MAX_HW_QUEUES", KGPU_HW_QUEUES_STR, 0);
    g_queues_ok = true;
    g_queues = KGPU_HW_QUEUES;
}
unsigned kgpu::planned_streams() {
    static const unsigned n = getenv("KGPU_STREAMS") && atoi(getenv("KGPU_STREAMS")) > 0 ? (unsigned)atoi(getenv("KGPU_STREAMS")) : (g_queues_ok ? 4u : 3u);
    return n;
}
// Streams for chains that start with the windowed kernel, beside the shared ones: what the hardware queues leave (16 queues: eight; 8: two; the default 4: none --
// such chains then stay on the shared streams).  KGPU_LONG_STREAMS overrides (0 = off).
unsigned kgpu::planned_long_streams() {
    static const unsigned n = [] {
        if (const char *e = getenv("KGPU_LONG_STREAMS")) return (unsigned)std::max(0, std::min(16, atoi(e)));
        const int spare = g_queues - 6;
        return (unsigned)std::max(0, std::min(8, spare));
    }();
    return n;
}

extern "C" int kgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------- dictionary

template <class T>
static int upload(kgpu_dict *d, const std::vector<T> &h, const T **out) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(h.size() * sizeof(T), 16);
    HIPCHECK(hipMalloc(&p, bytes));
    d->allocs.push_back(p);
    if (!h.empty()) HIPCHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    d->info.device_bytes += bytes;
    *out = (const T *)p;
    return KGPU_OK;
}

static int parse_morphs(Reader &r, std::vector<Morph8> &out, const char *what) {
    int64_t n = r.get<int64_t>();  // morph.rs:74-78
    if (r.bad || n < 0 || (uint64_t)n > r.left() / 6) { set_error("%s: truncated morph block", what); return KGPU_ERR_BAD_DICT; }
    out.resize((size_t)n);
    for (auto &m : out) { m.left = r.get<int16_t>(); m.right = r.get<int16_t>(); m.cost = r.get<int16_t>(); m.dup = 0; }
    return KGPU_OK;
}

extern "C" int kgpu_dict_create(const kgpu_dict_blobs *b, int device, kgpu_dict **out) {
    if (!b || !out) { set_error("kgpu_dict_create: null argument"); return KGPU_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!b->index_dict || !b->connection_dict || !b->morph_dict || !b->unk_dict || !b->char_category ||
        (!b->invoke_list && b->invoke_len) || (!b->group_list && b->group_len)) {
        set_error("kgpu_dict_create: null blob");
        return KGPU_ERR_INVALID_ARG;
    }
    // ---- parse (layouts: SURVEY.md App. B) ----
    std::vector<DaNode> da;
    std::vector<std::pair<int64_t, uint64_t>> dup;
    {
        Reader r(b->index_dict, b->index_len);  // trie/da.rs:220-236, index.rs:57-73
        uint64_t n = r.get<uint64_t>();
        if (r.bad || n > r.left() / 8 || n >= (1ull << 31)) { set_error("index.dict: bad double-array length"); return KGPU_ERR_BAD_DICT; }
        da.resize((size_t)n);
        if (n) { std::memcpy(da.data(), r.p + r.at, (size_t)n * 8); r.at += (size_t)n * 8; }
        uint64_t m = r.get<uint64_t>();
        if (r.bad || m > r.left() / 16) { set_error("index.dict: bad duplicate map"); return KGPU_ERR_BAD_DICT; }
        dup.resize((size_t)m);
        for (auto &kv : dup) { kv.first = r.get<int64_t>(); kv.second = r.get<uint64_t>(); }
    }
    // DoubleArray::search_common_prefix_of indexes self.0[1] unconditionally
    // (da.rs:156,161) and panics on a 1-element array (empty keyword list);
    // here such a trie simply matches nothing.
    while (da.size() < 2) da.push_back(DaNode{0, 0});

    uint64_t rows, cols;
    std::vector<int16_t> conn;
    {
        Reader r(b->connection_dict, b->connection_len);  // connection.rs:28-42
        rows = r.get<uint64_t>(); cols = r.get<uint64_t>();
        if (r.bad || rows >= (1ull << 31) || cols >= (1ull << 31) || (rows && cols > r.left() / 2 / rows)) {
            set_error("connection.dict: truncated"); return KGPU_ERR_BAD_DICT;
        }
        if (rows * cols >= (1ull << 32)) { set_error("connection.dict: matrix too large"); return KGPU_ERR_BAD_DICT; }
        conn.resize((size_t)(rows * cols));
        if (!conn.empty()) std::memcpy(conn.data(), r.p + r.at, conn.size() * 2);
    }
    std::vector<Morph8> morphs, unk_morphs;
    {
        Reader r(b->morph_dict, b->morph_len);
        int rc = parse_morphs(r, morphs, "morph.dict");
        if (rc) return rc;
    }
    std::vector<CatInfo> cinfo(256, CatInfo{0, 0, 0, 0});
    {
        Reader r(b->unk_dict, b->unk_len);  // unk_dict.rs:75-99
        uint64_t k = r.get<uint64_t>();
        if (r.bad || k > r.left() / 17) { set_error("unk.dict: truncated"); return KGPU_ERR_BAD_DICT; }
        struct E { uint8_t cat; int64_t first; uint64_t count; };
        std::vector<E> ents((size_t)k);
        for (auto &e : ents) { e.cat = r.get<uint8_t>(); e.first = r.get<int64_t>(); e.count = r.get<uint64_t>(); }
        int rc = parse_morphs(r, unk_morphs, "unk.dict");
        if (rc) return rc;
        for (auto &e : ents) {
            // lattice.rs:195 unk_dict.morphs[id - 1] must be in bounds for every id the entry yields
            if (e.count && (e.first < 1 || (uint64_t)e.first - 1 + e.count > unk_morphs.size())) {
                set_error("unk.dict: category %u maps to morph ids %lld..+%llu outside 1..%zu (reference would panic, lattice.rs:195)",
                          e.cat, (long long)e.first, (unsigned long long)e.count, unk_morphs.size());
                return KGPU_ERR_BAD_DICT;
            }
            cinfo[e.cat].flags |= CAT_HAS_UNK;
            cinfo[e.cat].unk_first = (int32_t)e.first;
            cinfo[e.cat].unk_count = (uint32_t)e.count;
        }
    }
    if (b->char_category_len == 0) { set_error("char_category: empty table (reference would panic, char_category_def.rs:37)"); return KGPU_ERR_BAD_DICT; }
    for (size_t i = 0; i < b->invoke_len && i < 256; ++i) if (b->invoke_list[i]) cinfo[i].flags |= CAT_INVOKE;
    for (size_t i = 0; i < b->group_len && i < 256; ++i) if (b->group_list[i]) cinfo[i].flags |= CAT_GROUP;
    {
        bool seen[256] = {false};
        for (size_t i = 0; i < b->char_category_len; ++i) seen[b->char_category[i]] = true;
        for (int c = 0; c < 256; ++c)
            if (seen[c] && (size_t)c >= b->invoke_len) {
                set_error("char_category: category %d has no invoke_list entry (reference would panic, lattice.rs:54)", c);
                return KGPU_ERR_BAD_DICT;
            }
    }
    // duplicate counts ride in the first record's padding
    for (auto &kv : dup) {
        if (kv.first < 1 || (uint64_t)kv.first > morphs.size() || kv.second > 65535 ||
            (uint64_t)kv.first + kv.second > morphs.size()) {
            set_error("index.dict: duplicate entry (%lld,+%llu) outside 1..%zu morphs", (long long)kv.first,
                      (unsigned long long)kv.second, morphs.size());
            return KGPU_ERR_BAD_DICT;
        }
        morphs[(size_t)kv.first - 1].dup = (uint16_t)kv.second;
    }
    // every leaf id (and its duplicates) must index morphs (lattice.rs:182)
    for (size_t a = 0; a < da.size(); ++a) {
        const DaNode &nd = da[a];
        if (nd.base < 0 && nd.check > 0 && (size_t)nd.check < da.size() && da[(size_t)nd.check].base == (int32_t)a) {
            int64_t id = -(int64_t)nd.base;
            if (id > (int64_t)morphs.size()) {
                set_error("index.dict: keyword id %lld has no morph (reference would panic, lattice.rs:182)", (long long)id);
                return KGPU_ERR_BAD_DICT;
            }
        }
    }
    // ConnectionTable::get(right, left) = data[rows*left + right] (connection.rs:12-14):
    // every (right, left) combination of the dictionary must stay in bounds.
    {
        int64_t max_l = 0, max_r = 0;
        auto scan = [&](const std::vector<Morph8> &v) {
            for (auto &m : v) {
                if (m.left < 0 || m.right < 0) return false;
                max_l = std::max<int64_t>(max_l, m.left); max_r = std::max<int64_t>(max_r, m.right);
            }
            return true;
        };
        if (!scan(morphs) || !scan(unk_morphs)) { set_error("morph: negative context id (reference would panic, connection.rs:13)"); return KGPU_ERR_BAD_DICT; }
        if ((uint64_t)max_l * rows + (uint64_t)max_r >= conn.size()) {
            set_error("connection.dict: %llux%llu matrix does not cover left_id %lld / right_id %lld (reference would panic, connection.rs:13)",
                      (unsigned long long)rows, (unsigned long long)cols, (long long)max_l, (long long)max_r);
            return KGPU_ERR_BAD_DICT;
        }
    }

    // ---- frequency-rank the context ids -------------------------------------------------
    // Context ids are only ever used to index the connection matrix (they are not part of a
    // Token), so they can be renumbered freely.  Ranking both id spaces by how many dictionary
    // records carry them puts the ids the lattice meets most often at the low indices: for a
    // target (one matrix row of 2.6 KB) all its frequent predecessors then sit in the row's first
    // cache line, and the frequent rows' first lines stay L1-resident.  The sweep's dominant L2
    // consumer is exactly this gather (connection.rs:12-14 once per relaxation).
    uint32_t bos_right = 0, eos_left = 0;
    std::vector<uint32_t> rank_r, rank_l;  // id -> rank, kept (inverted) for kgpu_lattice_dump
    {
        bool in_range = true;  // remap only when every id is a plain (row, col) index
        for (auto *v : {&morphs, &unk_morphs})
            for (auto &m : *v) if ((uint64_t)m.right >= rows || (uint64_t)m.left >= cols) in_range = false;
        if (in_range && rows && cols && rows < 65536 && cols < 65536) {
            std::vector<uint64_t> fr(rows, 0), fl(cols, 0);
            for (auto *v : {&morphs, &unk_morphs}) for (auto &m : *v) { fr[m.right]++; fl[m.left]++; }
            fr[0] += morphs.size(); fl[0] += morphs.size();  // BOS/EOS take part in every sentence
            auto rank = [](const std::vector<uint64_t> &f) {
                std::vector<uint32_t> order(f.size()), map(f.size());
                for (uint32_t i = 0; i < f.size(); ++i) order[i] = i;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return f[x] > f[y]; });
                for (uint32_t k = 0; k < order.size(); ++k) map[order[k]] = k;
                return map;
            };
            const std::vector<uint32_t> rmap = rank(fr), lmap = rank(fl);
            std::vector<int16_t> c2(conn.size());
            for (uint64_t l = 0; l < cols; ++l)
                for (uint64_t r = 0; r < rows; ++r) c2[(size_t)(lmap[l] * rows + rmap[r])] = conn[(size_t)(l * rows + r)];
            conn.swap(c2);
            for (auto *v : {&morphs, &unk_morphs})
                for (auto &m : *v) { m.right = (int16_t)rmap[m.right]; m.left = (int16_t)lmap[m.left]; }
            bos_right = rmap[0]; eos_left = lmap[0];
            rank_r = rmap; rank_l = lmap;
        }
    }

    // ---- the device copy of the double array carries the duplicate counts in its leaves ----
    // A leaf (reached through the terminator byte, trie/da.rs:118-123) stores base = -id.  The walk has to load that node
    // anyway, and the record count of the surface (index.rs:46-51) is the next thing it needs: with ids below 2^21 the spare
    // bits hold it (1023 = larger, look it up), and one dependent load per match disappears from the walk.
    const std::vector<DaNode> da_as_given(da);   // (the word counts' key table is built from the caller's own leaves, lazily)
    uint32_t leaf_dup = 0;
    if (morphs.size() < (1u << 21) && !test_hooks().plain_leaves /* tests: the layout of a dictionary with 2^21 morphs or more */) {
        leaf_dup = 1;
        for (size_t a2 = 0; a2 < da.size(); ++a2) {
            DaNode &nd = da[a2];
            if (nd.base < 0 && nd.check > 0 && (size_t)nd.check < da.size() && da[(size_t)nd.check].base == (int32_t)a2) {
                const uint32_t id = (uint32_t)(-(int64_t)nd.base);
                const uint32_t dupc = std::min<uint32_t>(morphs[id - 1].dup, 1023u);
                nd.base = -(int32_t)(id | (dupc << 21));
            }
        }
    }

    // ---- upload once to HBM ----
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("kgpu_dict_create: no HIP device (the HIP path has no CPU fallback)");
        return KGPU_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("kgpu_dict_create: device %d out of range (0..%d)", device, ndev - 1); return KGPU_ERR_INVALID_ARG; }
    HIPCHECK(hipSetDevice(device));
    kgpu_dict *d = new kgpu_dict();
    d->combiner = combiner_new();
    d->device = device;
    d->da_host = da_as_given;
    d->dup_host = dup;
    d->right_of_rank.resize(rank_r.size()); d->left_of_rank.resize(rank_l.size());
    for (uint32_t i = 0; i < rank_r.size(); ++i) d->right_of_rank[rank_r[i]] = i;
    for (uint32_t i = 0; i < rank_l.size(); ++i) d->left_of_rank[rank_l[i]] = i;
    std::vector<uint8_t> cat(b->char_category, b->char_category + b->char_category_len);
    int rc;
    // First-character jump table: the walk from every start position begins with a whole
    // character, so the 1-3 dependent node loads of its UTF-8 bytes (trie/da.rs:159-165) are
    // memoised per BMP code point.  Keys are UTF-8 strings, so no key ends inside a character.
    std::vector<DaNode> first(65536);
    for (uint32_t cp = 0; cp < 65536; ++cp) {
        uint8_t b[3]; int len;
        if (cp < 0x80) { b[0] = (uint8_t)cp; len = 1; }
        else if (cp < 0x800) { b[0] = 0xC0 | (cp >> 6); b[1] = 0x80 | (cp & 0x3F); len = 2; }
        else { b[0] = 0xE0 | (cp >> 12); b[1] = 0x80 | ((cp >> 6) & 0x3F); b[2] = 0x80 | (cp & 0x3F); len = 3; }
        int32_t pp = 1, steps = 0;
        bool ok = true;
        for (int k = 0; k < len; ++k) {
            ++steps;
            const int64_t q = (int64_t)da[(size_t)pp].base + b[k];
            if (q < 0 || q >= (int64_t)da.size() || da[(size_t)q].check != pp) { ok = false; break; }
            pp = (int32_t)q;
        }
        first[cp] = ok ? DaNode{pp, da[(size_t)pp].base} : DaNode{0, steps};
    }
    // Character-level copy of the trie (kgpu_chartrie.cpp): one dependent load per character instead of one per byte.
    CharTrie ct;
    const bool have_ct = !test_hooks().byte_trie && char_trie_buildable(da) && build_char_trie(da, cat.data(), cat.size(), ct);
    if (have_ct) {
        if ((rc = upload(d, ct.da, &d->view.da2)) || (rc = upload(d, ct.rec, &d->view.crec)) ||
            (rc = upload(d, ct.nb_cp, &d->view.nb_cp)) || (rc = upload(d, ct.nb_code, &d->view.nb_code))) {
            kgpu_dict_destroy(d);
            return rc;
        }
        d->view.da2_len = (uint32_t)ct.da.size();
        d->view.n_nb = (uint32_t)ct.nb_cp.size();
    }
    // ONE table for the known and the unknown words' records (DictView: unk_morph == morph + n_morph): a node's record is one index away whichever kind it is
    std::vector<Morph8> all_morphs(morphs);
    all_morphs.insert(all_morphs.end(), unk_morphs.begin(), unk_morphs.end());
    conn.resize(conn.size() + 2, 0);   // the pool kernel reads a cost with a dword load at its (2-byte-aligned) address: the last element's load stays inside the allocation
    if ((rc = upload(d, first, &d->view.first)) ||
        (rc = upload(d, da, &d->view.da)) || (rc = upload(d, all_morphs, &d->view.morph)) || (rc = upload(d, conn, &d->view.conn)) ||
        (rc = upload(d, cat, &d->view.cat)) || (rc = upload(d, cinfo, &d->view.cinfo))) {
        kgpu_dict_destroy(d);
        return rc;
    }
    d->view.da_len = (uint32_t)da.size();
    d->view.leaf_dup = leaf_dup;
    d->view.n_morph = (uint32_t)morphs.size();
    d->view.n_unk_morph = (uint32_t)unk_morphs.size();
    d->view.unk_morph = d->view.morph + morphs.size();
    d->view.conn_rows = (uint32_t)rows;
    d->view.bos_right = bos_right; d->view.eos_left = eos_left;
    d->view.cat_len = (uint32_t)std::min<size_t>(cat.size(), 0x110000);
    d->info.da_len = da.size(); d->info.n_morphs = morphs.size(); d->info.n_unk_morphs = unk_morphs.size();
    d->info.conn_rows = rows; d->info.conn_cols = cols; d->info.device = device;
    *out = d;
    g_err[0] = 0;
    if (planned_streams() < 4)   // not an error: the handle is good, the message is there for whoever looks
        set_error("warning: running on %u streams -- GPU_MAX_HW_QUEUES was %s when the HIP runtime initialised; set GPU_MAX_HW_QUEUES=16 in the environment "
                  "(or load this library before the first HIP call) for the full rate of concurrent batches", planned_streams(),
                  getenv("GPU_MAX_HW_QUEUES") ? "below 5" : "unset");
    return KGPU_OK;
}

extern "C" void kgpu_dict_destroy(kgpu_dict *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    std::vector<kgpu_ctx *> pooled;
    {
        std::lock_guard<std::mutex> g(d->pool_mu);
        pooled.swap(d->pool);
    }
    for (auto *c : pooled) kgpu_ctx_destroy(c);
    d->closed.store(true, std::memory_order_release);
    dict_release(d);
}

extern "C" int kgpu_dict_get_info(const kgpu_dict *d, kgpu_dict_info *out) {
    if (!d || !out) { set_error("kgpu_dict_get_info: null argument"); return KGPU_ERR_INVALID_ARG; }
    *out = d->info;
    return KGPU_OK;
}

extern "C" int kgpu_dict_get_routing(kgpu_dict *d, kgpu_routing *out, size_t out_size, int reset) {
    if (!d || !out || out_size < 8) { set_error("kgpu_dict_get_routing: bad argument"); return KGPU_ERR_INVALID_ARG; }
    kgpu_routing sum{};
    {
        std::lock_guard<std::mutex> g(d->pool_mu);
        for (kgpu_ctx *c : d->pool) {
            const kgpu_routing &r = c->rt;
            sum.batches += r.batches; sum.sentences += r.sentences;
            for (int k = 0; k < 4; ++k) { sum.deferred[k] += r.deferred[k]; sum.redone[k] += r.redone[k]; }
            sum.long_launches += r.long_launches; sum.arena_regrows += r.arena_regrows; sum.first_ms += r.first_ms;
            sum.small_calls += r.small_calls; sum.small_fallbacks += r.small_fallbacks; sum.window_reruns += r.window_reruns; sum.tail_reruns += r.tail_reruns;
            sum.combined_calls += r.combined_calls; sum.combined_launches += r.combined_launches;
            for (int k = 0; k < 10; ++k) sum.window_handed[k] += r.window_handed[k];
            if (reset) c->rt = kgpu_routing{};
        }
    }
    std::memcpy(out, &sum, std::min(out_size, sizeof sum));
    return KGPU_OK;
}
