// kanpyo_amd/csrc/kgpu_count.hip -- the word counts of a batch on the device (include/kanpyo_gpu.h, "word counts"; not an output of the reference):
// every token the wakati render would keep adds one to its word's 64-bit counter in a counts handle (kgpu_count_host.cpp).  Nothing but two words
// returns to the host.
//
// Two launches on the context's stream:
//   k_count_words    one wavefront per sentence, 64 records at a time; the walk, the record check and a record's word are the renders' (kgpu_records_dev.h).
//       ROW-DETERMINED words (a known token with a row; a pool name) are counted per feature row.  Natural text puts a large share of its tokens on a few
//       particles, and one word of global memory takes about 90 atomic operations per microsecond chip-wide (kgpu_device.h, above WorkIO): the workgroup
//       sums in LDS first -- a table of LH entries keyed by the row, claimed with a compare-and-swap, summed with LDS adds -- and adds every distinct row
//       to the handle's dense counters ONCE, when it is through.  A row that finds no entry within LDS_PROBES steps goes to its dense counter directly.
//       EVERY OTHER WORD (an unknown-class surface, the surface of a token without a row) goes to the byte-keyed table.  It is wait-free:
//         1. the lane probes read-only from hash & mask: a slot whose tag carries the hash and whose arena entry holds the same length and bytes is the
//            word's -- one atomic add, done; a free slot ends the probe.  Only words that are new pay for arena space;
//         2. the lanes of the wavefront that met a free slot take their arena space together (one add to the cursor per wavefront), write their
//            entries whole -- length, hash, bytes -- and only then try to claim the slot with a compare-and-swap (release: the entry is visible
//            to whoever reads the tag with acquire);
//         3. a lane that loses the swap looks at what won: the same word -- it adds there, its own entry stays unused --, another -- it walks on.
//       No lane ever waits for another: every loop is bounded by the table's size.  A word that finds no slot or no arena space is counted in the
//       handle's overflow tokens.  Bytes are hashed and compared one at a time from wherever they lie: any alignment, any length, nothing read past them.
//   k_count_publish  one workgroup: the launch's per-workgroup totals summed into the handle's words and published to the host.
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = 8;          // wavefronts per workgroup (one sentence each at a time)
constexpr uint32_t MAX_BLOCKS = 256; // a hot row costs one global add per workgroup: few, large workgroups
constexpr uint32_t LH = 1024;        // entries of the workgroup's LDS table
constexpr uint32_t LDS_PROBES = 8;

__device__ __forceinline__ void entry_write(uint8_t *e, uint32_t h, const uint8_t *p, uint32_t len) {
    *(uint2 *)e = make_uint2(len, h);
    for (uint32_t i = 0; i < len; i += 8) {
        const uint32_t m = len - i < 8 ? len - i : 8;
        unsigned long long v = 0;
        for (uint32_t b = 0; b < m; ++b) v |= (unsigned long long)p[i + b] << (8 * b);
        *(unsigned long long *)(e + COUNT_ENTRY_HEAD + i) = v;
    }
}

enum : int { WALK_DONE = 0, WALK_FREE = 1, WALK_FULL = 2 };
// The probe from slot i on (`probes` slots seen so far).  tag == 0: read-only, a free slot ends it (WALK_FREE, i is that slot).  tag != 0: the lane's own
// entry is written: a free slot is claimed with it.  WALK_DONE: the word's counter has its one more.  WALK_FULL: every slot holds another word.
__device__ __forceinline__ int table_walk(const CountsArgs &a, const uint8_t *p, uint32_t len, uint32_t h, uint32_t &i, uint32_t &probes,
                                          unsigned long long tag, uint32_t &claimed) {
    for (; probes <= a.slot_mask; ++probes, i = (i + 1) & a.slot_mask) {
        CountSlot &sl = a.slots[i];
        unsigned long long t = __hip_atomic_load(&sl.tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (t == 0) {
            if (tag == 0) return WALK_FREE;
            if (__hip_atomic_compare_exchange_strong(&sl.tag, &t, tag, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) {
                ++claimed;
                (void)__hip_atomic_fetch_add(&sl.count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return WALK_DONE;
            }
            // lost: t is what won -- compared like any other occupied slot
        }
        if ((uint32_t)(t >> 32) == h && entry_equals(a.arena + ((t & 0xFFFFFFFFull) - 1) * 8, h, p, len)) {
            (void)__hip_atomic_fetch_add(&sl.count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return WALK_DONE;
        }
    }
    return WALK_FULL;
}

__device__ __forceinline__ void lds_add(uint32_t *hk, unsigned long long *hc, unsigned long long *dense, uint32_t row) {
    const uint32_t key = row + 1;
    uint32_t h = (key * 2654435761u) >> 22;
    static_assert(LH == 1u << 10, "the shift above");
    for (uint32_t p = 0; p < LDS_PROBES; ++p, h = (h + 1) & (LH - 1)) {
        uint32_t cur = __hip_atomic_load(&hk[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) { cur = atomicCAS(&hk[h], 0u, key); if (cur == 0) cur = key; }
        if (cur == key) { atomicAdd(&hc[h], 1ull); return; }
    }
    atomicAdd(&dense[row], 1ull);   // the workgroup's table is crowded around this row: straight to its counter
}

}  // namespace

__global__ __launch_bounds__(64 * WPB) void k_count_words(CountsArgs a) {
    __shared__ uint32_t hk[LH];
    __shared__ unsigned long long hc[LH];
    __shared__ unsigned long long tot[COUNT_PARTIAL_WORDS];
    for (uint32_t i = threadIdx.x; i < LH; i += blockDim.x) { hk[i] = 0; hc[i] = 0; }
    if (threadIdx.x < COUNT_PARTIAL_WORDS) tot[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    uint64_t cnt_all = 0, ovf_all = 0;
    uint32_t claimed_all = 0;
    const bool anybad = walk_sentences<WPB, true>(a.b, [&](uint64_t, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        uint64_t cnt = 0, ovf = 0;   // (the sentence's own: tallies captured by reference would live in scratch memory)
        uint32_t claimed = 0;
        bool bad = false;
        for (uint64_t kw = k0; kw < k1; kw += 64) {   // (wave-uniform)
            Word wd{0, 0, true, false, true};
            kgpu_token t{};
            if (kw + lane < k1) { t = a.b.tokens[kw + lane]; wd = word_of(a.b, a.w, t, B); }
            bad |= !wd.ok;
            bool need = false;
            uint32_t h = 0, i = 0, probes = 0;
            const uint8_t *p = text + wd.src;
            if (wd.kept) {
                if (row_determined(t, wd)) {
                    lds_add(hk, hc, a.dense, feature_row(t.cls == KGPU_CLASS_KNOWN, a.b.n_morph, (uint32_t)t.id));
                    ++cnt;
                } else {
                    h = key_hash(p, wd.len);
                    i = h & a.slot_mask;
                    const int r = table_walk(a, p, wd.len, h, i, probes, 0, claimed);
                    if (r == WALK_DONE) ++cnt;
                    else if (r == WALK_FULL) ++ovf;
                    else need = true;
                }
            }
            uint64_t size = need ? COUNT_ENTRY_HEAD + (((uint64_t)wd.len + 7) & ~7ull) : 0;
            if (need && __hip_atomic_load(&a.stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + size > a.arena_bytes) {
                need = false; size = 0; ++ovf;   // (the cursor only grows: this key cannot fit, and does not take the room of keys that can)
            }
            if (__ballot(need) != 0) {   // (wave-uniform) new words: one add to the arena cursor for the wavefront
                const uint64_t incl = wave_incl_scan64(size, lane);
                const uint64_t total = lane63(incl);
                uint64_t base = 0;
                if (lane == 0) base = atomicAdd(&a.stats[0], (unsigned long long)total);
                base = bcast64(base);
                if (need) {
                    const uint64_t off = base + incl - size;
                    if (off + size <= a.arena_bytes) {
                        entry_write(a.arena + off, h, p, wd.len);
                        const unsigned long long tag = ((unsigned long long)h << 32) | (off / 8 + 1);
                        if (table_walk(a, p, wd.len, h, i, probes, tag, claimed) == WALK_DONE) ++cnt;
                        else ++ovf;
                    } else {
                        ++ovf;
                    }
                }
            }
        }
        cnt_all += cnt; ovf_all += ovf; claimed_all += claimed;
        return bad;
    });
    const uint64_t cnt = wave_sum64(cnt_all), ovf = wave_sum64(ovf_all), cl = wave_sum64((uint64_t)claimed_all);
    if (lane == 0) {
        if (cnt) atomicAdd(&tot[0], (unsigned long long)cnt);
        if (ovf) atomicAdd(&tot[1], (unsigned long long)ovf);
        if (anybad) atomicAdd(&tot[2], 1ull);
        if (cl) atomicAdd(&tot[3], (unsigned long long)cl);
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < LH; e += blockDim.x)
        if (hk[e] != 0) atomicAdd(&a.dense[hk[e] - 1], hc[e]);   // every distinct row of the workgroup: once
    if (threadIdx.x < COUNT_PARTIAL_WORDS) a.b.sent_len[(uint64_t)blockIdx.x * COUNT_PARTIAL_WORDS + threadIdx.x] = tot[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_count_publish(CountsArgs a, uint32_t blocks) {
    __shared__ unsigned long long sum[COUNT_PARTIAL_WORDS];
    if (threadIdx.x < COUNT_PARTIAL_WORDS) sum[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < blocks * COUNT_PARTIAL_WORDS; k += blockDim.x) {
        const unsigned long long v = a.b.sent_len[k];
        if (v) atomicAdd(&sum[k % COUNT_PARTIAL_WORDS], v);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sum[3]) atomicAdd(&a.stats[1], sum[3]);
        if (sum[0]) atomicAdd(&a.stats[2], sum[0]);
        if (sum[1]) atomicAdd(&a.stats[3], sum[1]);
        __hip_atomic_store(&a.b.host_ctl[0], sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.b.host_ctl[1], (sum[2] ? 1ull : 0ull) | (sum[1] ? 2ull : 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

uint32_t count_blocks(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + WPB - 1) / WPB, MAX_BLOCKS)); }

int launch_count_words(const CountsArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = count_blocks(a.b.n);
    hipLaunchKernelGGL(k_count_words, dim3(blocks), dim3(64 * WPB), 0, st, a);
    hipLaunchKernelGGL(k_count_publish, dim3(1), dim3(256), 0, st, a, blocks);
    return (int)hipGetLastError();
}

}  // namespace kgpu
