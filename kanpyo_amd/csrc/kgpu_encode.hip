// kanpyo_amd/csrc/kgpu_encode.hip -- the vocabulary ids of a batch on the device (include/kanpyo_gpu.h, "vocabulary ids"; not an output of the
// reference): every token the wakati render would keep gives ONE int32, the index of its word in a vocabulary handle's list (kgpu_encode_host.cpp), or
// the handle's unk_id.  A sentence's sequence is [bos] ids... [eos]; ragged (back to back, id_offsets in ids) or padded (n x width, pad_id behind).
//
// Three launches on the context's stream, the shape of kgpu_words.hip:
//   k_encode_len    one wavefront per sentence: its kept tokens + bos + eos -> sent_len[s]; records are range-checked as word_of checks them,
//                   the status bytes mirrored
//   k_lines_scan    kgpu_format.hip's, unchanged: exclusive scan (the units are ids), mirrored into the caller's id_offsets, the total published
//   k_encode_write  one wavefront per sentence, 64 records at a time: a kept lane's rank is a ballot and a prefix count, its id ONE load from row_id
//                   when the word is row-determined (the count kernel's predicate: a known token with a row, a pool name) and otherwise a READ-ONLY
//                   probe of the frozen byte-keyed table -- plain loads, the key hashed and compared one byte at a time from the text: any alignment,
//                   nothing read past it; every probe loop is bounded by the table.  The lane stores one int32 at base + rank: a window's stores are
//                   consecutive dwords.  Lane 0 writes bos and eos.  Ragged: nothing at all is written when the total exceeds the capacity.
//                   Padded: the sentence's base is s * width, the windows stop once the row is full, [min(L, width), width) is filled with pad_id
//                   and a truncated row ends with eos_id when EOS was asked for.  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_words_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = 4;   // wavefronts per workgroup (one sentence each at a time)

// The id of the len bytes at p: the slot whose tag carries the hash and whose arena entry holds the same length and bytes; a free slot ends the probe.
__device__ __forceinline__ int32_t vocab_lookup(const EncodeArgs &a, const uint8_t *p, uint32_t len) {
    const uint32_t h = key_hash(p, len);
    uint32_t i = h & a.slot_mask;
    for (uint64_t probes = 0; probes <= a.slot_mask; ++probes, i = (i + 1) & a.slot_mask) {   // (64-bit: bounded at 2^32 slots too)
        const uint4 sl = *(const uint4 *)&a.slots[i];   // tag (x, y), id (z)
        if ((sl.x | sl.y) == 0) break;
        if (sl.y == h && entry_equals(a.arena + ((uint64_t)sl.x - 1) * 8, h, p, len)) return (int32_t)sl.z;
    }
    return a.unk_id;
}

}  // namespace

__global__ __launch_bounds__(256) void k_encode_len(EncodeArgs a) {
    const WordsArgs &w = a.w;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t extra = ((a.flags & VOCAB_BOS) ? 1u : 0u) + ((a.flags & VOCAB_EOS) ? 1u : 0u);
    bool bad = false;
    for (uint64_t s = wave; s < w.n; s += nwaves) {
        const uint64_t k0 = w.tok_offsets[s], k1 = w.tok_offsets[s + 1];
        const uint32_t B = (uint32_t)(w.offsets[s + 1] - w.offsets[s]);
        bad |= k1 < k0;
        uint64_t cnt = 0;
        for (uint64_t k = k0 + lane; k < k1; k += 64) {
            const Word wd = word_of(w, w.tokens[k], B);
            cnt += wd.kept ? 1u : 0u;
            bad |= !wd.ok;
        }
        cnt = wave_sum64(cnt);
        if (lane == 0) {
            w.sent_len[s] = cnt + extra;
            if (w.status_out) w.status_out[s] = w.status_in[s];
        }
    }
    if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&w.host_ctl[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_encode_write(EncodeArgs a) {
    const WordsArgs &w = a.w;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t *ioff = w.sent_len;    // the scan's offsets in device memory
    const bool padded = a.width != 0;
    if (!padded && ioff[w.n] > a.id_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const bool bos = (a.flags & VOCAB_BOS) != 0, eos = (a.flags & VOCAB_EOS) != 0;
    for (uint64_t s = wave; s < w.n; s += nwaves) {
        const uint64_t k0 = w.tok_offsets[s], k1 = w.tok_offsets[s + 1];
        const uint64_t L = ioff[s + 1] - ioff[s];   // the untruncated sequence
        const uint8_t *text = w.utf8 + w.offsets[s];
        const uint32_t B = (uint32_t)(w.offsets[s + 1] - w.offsets[s]);
        int32_t *const row = a.ids + (padded ? s * a.width : ioff[s]);
        // the slots bos and the kept tokens may take: a truncated row keeps its last slot for eos (no two lanes ever store to one slot)
        const uint64_t lim = !padded ? L : (L > a.width ? a.width - (eos ? 1u : 0u) : L);
        uint64_t at = 0;   // (wave-uniform) elements of the sequence placed so far
        if (bos) {
            if (lane == 0 && lim > 0) row[0] = a.bos_id;
            at = 1;
        }
        for (uint64_t kw = k0; kw < k1 && at < lim; kw += 64) {   // (wave-uniform) padded: the windows stop once the row is full
            Word wd{0, 0, true, false, true};
            kgpu_token t{};
            if (kw + lane < k1) { t = w.tokens[kw + lane]; wd = word_of(w, t, B); }
            const unsigned long long keep = __ballot(wd.kept);
            if (keep == 0) continue;   // (wave-uniform)
            const uint64_t slot = at + (uint32_t)__popcll(keep & ((1ull << lane) - 1));
            if (wd.kept && slot < lim) {
                int32_t id;
                if (t.id != 0 && (t.cls == KGPU_CLASS_KNOWN || !wd.from_text))   // row-determined (word_of has checked the id)
                    id = a.row_id[(t.cls == KGPU_CLASS_KNOWN ? 0u : w.n_morph) + (uint32_t)t.id - 1];
                else
                    id = vocab_lookup(a, text + wd.src, wd.len);
                row[slot] = id;
            }
            at += (uint32_t)__popcll(keep);
        }
        if (eos && lane == 0) row[(padded && L > a.width ? a.width : L) - 1] = a.eos_id;
        if (padded)
            for (uint64_t j = L + lane; j < a.width; j += 64) row[j] = a.pad_id;
    }
}

int launch_encode(const EncodeArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.w.n + WPB - 1) / WPB, 8192));
    hipLaunchKernelGGL(k_encode_len, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    LinesArgs sc{};   // what k_lines_scan reads and writes
    sc.n = a.w.n; sc.sent_len = a.w.sent_len; sc.text_offsets = a.w.text_offsets; sc.host_ctl = a.w.host_ctl;
    launch_lines_scan(sc, stream);
    hipLaunchKernelGGL(k_encode_write, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
