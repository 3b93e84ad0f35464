// kanpyo_amd/csrc/kgpu_encode.hip -- the vocabulary ids of a batch on the device (include/kanpyo_gpu.h, "vocabulary ids"; not an output of the
// reference): every token the wakati render would keep gives ONE int32, the index of its word in a vocabulary handle's list (kgpu_encode_host.cpp), or
// the handle's unk_id.  A sentence's sequence is [bos] ids... [eos]; ragged (back to back, id_offsets in ids) or padded (n x width, pad_id behind).
//
// Three launches on the context's stream (kgpu_records_dev.h: launch_render):
//   k_encode_len    sentence_units: a kept token gives one id; bos and eos are added to the sum
//   k_lines_scan    kgpu_format.hip's: the scan's mirror is the caller's id_offsets
//   k_encode_write  one wavefront per sentence, 64 records at a time: a kept lane's rank is a ballot and a prefix count, its id ONE load from row_id
//                   when the word is row-determined and otherwise a READ-ONLY
//                   probe of the frozen byte-keyed table -- plain loads, the key hashed and compared one byte at a time from the text: any alignment,
//                   nothing read past it; every probe loop is bounded by the table.  The lane stores one int32 at base + rank: a window's stores are
//                   consecutive dwords.  Lane 0 writes bos and eos.  Ragged: nothing at all is written when the total exceeds the capacity.
//                   Padded: the sentence's base is s * width, the windows stop once the row is full, [min(L, width), width) is filled with pad_id
//                   and a truncated row ends with eos_id when EOS was asked for.  All offsets are 64-bit.
//
// k_encode_write is a template on SPANS.  <false> is the kernel above, statement for statement.  <true> (include/kanpyo_gpu.h, "ids with spans"; its
// argument type derives from EncodeArgs, the length pass and the scan are the same launches) stores, wherever a lane stores an id, the element's source
// span as ONE 16-byte store and its token index at the same slot under the same bound (kgpu_spans_dev.h): a kept token's own four fields, mapped through
// the sentence's edits when the caller gave them; zeros and -1 for bos, eos and pad.
#include <type_traits>

#include "kgpu_spans_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = RENDER_WPB;

// The id of the len bytes at p: the slot whose tag carries the hash and whose arena entry holds the same length and bytes; a free slot ends the probe.
__device__ __forceinline__ int32_t vocab_lookup(const EncodeArgs &a, const uint8_t *p, uint32_t len) {
    return table_lookup(a, key_hash(p, len), p, len, a.unk_id);   // (kgpu_records_dev.h: the probe loop, shared with kgpu_wordpiece.hip)
}

}  // namespace

__global__ __launch_bounds__(256) void k_encode_len(EncodeArgs a) {
    const uint64_t extra = ((a.flags & VOCAB_BOS) ? 1u : 0u) + ((a.flags & VOCAB_EOS) ? 1u : 0u);
    sentence_units(a.b, [&](const kgpu_token &t, uint32_t B) { const Word w = word_of(a.b, a.w, t, B); return Units{w.kept ? 1u : 0u, w.ok}; },
                   [&](uint64_t sum) { return sum + extra; });
}

template <bool SPANS>
__global__ __launch_bounds__(256) void k_encode_write(std::conditional_t<SPANS, EncodeSpanArgs, EncodeArgs> a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t *ioff = a.b.sent_len;    // the scan's offsets in device memory
    const bool padded = a.width != 0;
    if (!padded && ioff[a.b.n] > a.id_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const bool bos = (a.flags & VOCAB_BOS) != 0, eos = (a.flags & VOCAB_EOS) != 0;
    walk_sentences<WPB, false>(a.b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        const uint64_t L = ioff[s + 1] - ioff[s];   // the untruncated sequence
        int32_t *const row = a.ids + (padded ? s * a.width : ioff[s]);
        // the slots bos and the kept tokens may take: a truncated row keeps its last slot for eos (no two lanes ever store to one slot)
        const uint64_t lim = !padded ? L : (L > a.width ? a.width - (eos ? 1u : 0u) : L);
        [[maybe_unused]] SpanRow sr{};   // (SPANS) the sentence's span and token-index rows, element for element beside `row`
        if constexpr (SPANS) sr = span_row(a.o, s, padded ? s * a.width : ioff[s]);
        uint64_t at = 0;   // (wave-uniform) elements of the sequence placed so far
        if (bos) {
            if (lane == 0 && lim > 0) {
                row[0] = a.bos_id;
                if constexpr (SPANS) span_special(sr, 0);
            }
            at = 1;
        }
        for (uint64_t kw = k0; kw < k1 && at < lim; kw += 64) {   // (wave-uniform) padded: the windows stop once the row is full
            Word wd{0, 0, true, false, true};
            kgpu_token t{};
            if (kw + lane < k1) { t = a.b.tokens[kw + lane]; wd = word_of(a.b, a.w, t, B); }
            const unsigned long long keep = __ballot(wd.kept);
            if (keep == 0) continue;   // (wave-uniform)
            const uint64_t slot = at + (uint32_t)__popcll(keep & ((1ull << lane) - 1));
            if (wd.kept && slot < lim) {
                row[slot] = row_determined(t, wd) ? a.row_id[feature_row(t.cls == KGPU_CLASS_KNOWN, a.b.n_morph, (uint32_t)t.id)] : vocab_lookup(a, text + wd.src, wd.len);
                if constexpr (SPANS) span_store(sr, slot, t.position, t.byte_len, t.start, t.end, (int32_t)(kw + lane - k0));   // the record's place in its sentence
            }
            at += (uint32_t)__popcll(keep);
        }
        if (eos && lane == 0) {
            row[(padded && L > a.width ? a.width : L) - 1] = a.eos_id;
            if constexpr (SPANS) span_special(sr, (padded && L > a.width ? a.width : L) - 1);
        }
        if (padded)
            for (uint64_t j = L + lane; j < a.width; j += 64) {
                row[j] = a.pad_id;
                if constexpr (SPANS) span_special(sr, j);
            }
        return false;   // (the length pass has checked the records)
    });
}

int launch_encode(const EncodeArgs &a, void *stream) { return launch_render(k_encode_len, k_encode_write<false>, a, stream); }
int launch_encode_spans(const EncodeSpanArgs &a, void *stream) { return launch_render(k_encode_len, k_encode_write<true>, a, stream); }

}  // namespace kgpu
