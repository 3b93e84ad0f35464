// kanpyo_amd/csrc/kgpu_wordpiece.hip -- the WordPiece ids of a batch on the device (include/kanpyo_gpu.h, "WordPiece ids"; not an output of the reference):
// every token the wakati render would keep gives the greedy longest-match pieces of its word over a WordPiece handle's two frozen tables
// (kgpu_wordpiece_table.cpp) -- none for the empty word, [unk_id] for a word that is too long or that no sequence of listed pieces spells.  A sentence's
// sequence is [bos] pieces... [eos]; ragged or padded exactly as kgpu_encode.hip's.  A plain vocabulary never comes here (kgpu_encode_host.cpp: enqueue_encode).
//
// Three launches on the context's stream (kgpu_records_dev.h: launch_render):
//   k_wordpiece_len    sentence_units: a kept token gives its row's count when its word is row-determined (the host has split it once), else what
//                      wordpiece_match counts; bos and eos are added to the sum
//   k_lines_scan       kgpu_format.hip's: the scan's mirror is the caller's id_offsets
//   k_wordpiece_write  one wavefront per sentence, 64 records at a time: a lane's first slot is `at` plus the wavefront's EXCLUSIVE prefix sum of the window's
//                      per-lane counts (the DPP scan of kgpu_device.h: a lane gives 0 .. max_word_chars units, so no ballot can rank it); the lane stores element
//                      j at row[slot + j] while slot + j < lim -- a padded row may be cut inside a token's pieces.  A row-determined lane copies the inline id
//                      or its run of the pool; a text-keyed lane whose match gave ONE id stores that id, and one that gave several runs wordpiece_match a
//                      second time and stores as it goes (the first run has shown that the match succeeds: nothing stored is ever taken back).
//                      bos, eos, the pad fill and the ragged "nothing at all when the total exceeds the capacity" are k_encode_write's.  All offsets are 64-bit.
//
// wordpiece_match is ONE template for both passes: the length pass and the write pass cannot disagree.  Every loop in it is bounded by the word's length, by
// max_word_chars and by the tables; every probe is a read-only table_lookup; nothing is read past the word.
//
// k_wordpiece_write is a template on SPANS.  <false> is the kernel above, statement for statement.  <true> (include/kanpyo_gpu.h, "ids with spans"; its
// argument type derives from WordpieceArgs, the length pass and the scan are the same launches) stores beside every id the element's source span (ONE
// 16-byte store) and its token index, at the same slot under the same bound (kgpu_spans_dev.h).  Piece j of a surface word that splits covers its own
// bytes and characters of the token: a text-keyed lane has them from the match (wordpiece_match<true> hands emit the piece's byte and character range:
// `start`, `best_len` and the count of the character ends it walked past), a row-determined lane from the pool of ends beside piece_ids, and only when
// the row's word is the surface and as long as the record says (the last piece ends where the word ends).  Every other element has the token's whole span.
#include <type_traits>

#include "kgpu_spans_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = RENDER_WPB;
constexpr int32_t NO_ID = -1;   // (list indices are never negative)

struct Match { uint32_t count; int32_t id; };   // count pieces; count == 1: `id` is the one (a listed entry, or unk_id)

// The split of the len bytes at p.  emit(j, id) -- ENDS: emit(j, id, b, e, cb, ce), the piece being bytes [b, e) and characters [cb, ce) of the word -- is
// called for piece j = 0, 1, ... as it is found -- on a word that turns out to have no split the pieces
// emitted so far are void: the caller that stores them asks with a no-op emit first.  -> the count the word gives and, for a count of one, its id.
//   1. the characters are counted first (a character starts at byte 0 and at every byte that is not 10xxxxxx) and the count stops at max_chars + 1: a
//      1024-character unknown run costs max_chars + 1 characters' bytes here and no probe at all
//   2. for each start the bytes are walked forward ONCE, no further than the table's longest entry, carrying the FNV-1a state; at every character start (and
//      at the word's end) the state is finished with the prefix's length and the prefix probed; the last hit is the longest
template <bool ENDS = false, class E>
__device__ __forceinline__ Match wordpiece_match(const WordpieceArgs &a, const uint8_t *p, uint32_t len, E &&emit) {
    if (len == 0) return Match{0, NO_ID};
    uint32_t chars = 0;
    for (uint32_t i = 0; i < len && chars <= a.max_chars; ++i) chars += (i == 0 || (p[i] & 0xC0u) != 0x80u) ? 1u : 0u;
    if (chars > a.max_chars) return Match{1, a.unk_id};
    uint32_t start = 0, n = 0;
    [[maybe_unused]] uint32_t cstart = 0;   // (ENDS) the characters in front of `start`
    int32_t last = NO_ID;
    while (start < len && n < chars) {   // (a piece is a character at least: n < chars never ends the loop first)
        const ByteTable &tb = start == 0 ? a.initial : a.cont;
        const uint32_t left = len - start, lim = left < tb.max_bytes ? left : tb.max_bytes;
        const uint8_t *q = p + start;
        uint32_t h = KEY_HASH_INIT, best_len = 0;
        int32_t best = NO_ID;
        [[maybe_unused]] uint32_t seen = 0, best_chars = 0;   // (ENDS) character ends walked past: the characters of the prefix probed; those of the longest hit
        for (uint32_t k = 0; k < lim; ++k) {
            h = key_hash_step(h, q[k]);
            const uint32_t e = k + 1;
            if (e < left && (q[e] & 0xC0u) == 0x80u) continue;   // inside a character: no piece ends here
            if constexpr (ENDS) ++seen;
            const int32_t id = table_lookup(tb, key_hash_finish(h, e), q, e, NO_ID);
            if (id != NO_ID) {
                best = id; best_len = e;
                if constexpr (ENDS) best_chars = seen;
            }
        }
        if (best == NO_ID) return Match{1, a.unk_id};   // no piece starts here: the WHOLE word is unk_id
        if constexpr (ENDS) emit(n, best, start, start + best_len, cstart, cstart + best_chars);
        else emit(n, best);
        last = best;
        ++n;
        start += best_len;
        if constexpr (ENDS) cstart += best_chars;
    }
    return Match{n, last};
}

struct NoEmit { __device__ __forceinline__ void operator()(uint32_t, int32_t) const {} };

}  // namespace

__global__ __launch_bounds__(256) void k_wordpiece_len(WordpieceArgs a) {
    const uint64_t extra = ((a.flags & VOCAB_BOS) ? 1u : 0u) + ((a.flags & VOCAB_EOS) ? 1u : 0u);
    sentence_units(a.b, [&](const kgpu_token &t, uint32_t B, const uint8_t *text) {
        const Word w = word_of(a.b, a.w, t, B);
        if (!w.kept) return Units{0, w.ok};
        if (row_determined(t, w)) return Units{a.rows[feature_row(t.cls == KGPU_CLASS_KNOWN, a.b.n_morph, (uint32_t)t.id)].count, true};
        return Units{wordpiece_match(a, text + w.src, w.len, NoEmit{}).count, true};
    }, [&](uint64_t sum) { return sum + extra; });
}

template <bool SPANS>
__global__ __launch_bounds__(256) void k_wordpiece_write(std::conditional_t<SPANS, WordpieceSpanArgs, WordpieceArgs> a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t *ioff = a.b.sent_len;    // the scan's offsets in device memory
    const bool padded = a.width != 0;
    if (!padded && ioff[a.b.n] > a.id_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const bool bos = (a.flags & VOCAB_BOS) != 0, eos = (a.flags & VOCAB_EOS) != 0;
    walk_sentences<WPB, false>(a.b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        const uint64_t L = ioff[s + 1] - ioff[s];   // the untruncated sequence
        int32_t *const row = a.ids + (padded ? s * a.width : ioff[s]);
        // the slots bos and the pieces may take: a truncated row keeps its last slot for eos (no two lanes ever store to one slot)
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
            uint32_t cnt = 0, first = 0;   // this lane's units; first: the id itself (cnt == 1), or where its run of the pool starts (row-determined, cnt > 1)
            bool by_row = false;
            if (kw + lane < k1) {
                t = a.b.tokens[kw + lane];
                wd = word_of(a.b, a.w, t, B);
                if (wd.kept) {
                    by_row = row_determined(t, wd);
                    if (by_row) {
                        const uint2 e = *(const uint2 *)&a.rows[feature_row(t.cls == KGPU_CLASS_KNOWN, a.b.n_morph, (uint32_t)t.id)];
                        first = e.x; cnt = e.y;
                    } else {
                        const Match m = wordpiece_match(a, text + wd.src, wd.len, NoEmit{});
                        first = (uint32_t)m.id; cnt = m.count;
                    }
                }
            }
            const uint32_t incl = wave_incl_scan(cnt, lane);   // (exec is full here: the loop is wave-uniform; a window's total is at most 64 x 1024)
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total == 0) continue;   // (wave-uniform)
            const uint64_t slot = at + (incl - cnt);
            [[maybe_unused]] const int32_t ti = (int32_t)(kw + lane - k0);   // (SPANS) the record's place in its sentence
            if (cnt == 1) {
                if (slot < lim) {
                    row[slot] = (int32_t)first;
                    if constexpr (SPANS) span_store(sr, slot, t.position, t.byte_len, t.start, t.end, ti);
                }
            } else if (cnt > 1 && slot < lim) {
                const uint64_t room = lim - slot;   // elements of this lane's that the row still takes
                if (by_row) {
                    const uint32_t m = cnt < room ? cnt : (uint32_t)room;
                    if constexpr (!SPANS) {
                        for (uint32_t j = 0; j < m; ++j) row[slot + j] = a.piece_ids[(uint64_t)first + j];
                    } else {
                        // the pool's ends hold for a row whose word is the surface, and for a record as long as that word: the last piece ends where the word ends
                        const bool own = wd.from_text && a.piece_ends[(uint64_t)first + cnt - 1].byte_end == t.byte_len;
                        uint32_t b = 0, cb = 0;   // where piece j starts in the word
                        for (uint32_t j = 0; j < m; ++j) {
                            row[slot + j] = a.piece_ids[(uint64_t)first + j];
                            if (own) {
                                const uint2 e = *(const uint2 *)&a.piece_ends[(uint64_t)first + j];
                                span_store(sr, slot + j, t.position + b, e.x - b, t.start + cb, t.start + e.y, ti);
                                b = e.x; cb = e.y;
                            } else {
                                span_store(sr, slot + j, t.position, t.byte_len, t.start, t.end, ti);
                            }
                        }
                    }
                } else if constexpr (!SPANS) {
                    wordpiece_match(a, text + wd.src, wd.len, [&](uint32_t j, int32_t id) { if (j < room) row[slot + j] = id; });
                } else {   // (a text-keyed word is the record's own bytes: wd.len == t.byte_len)
                    wordpiece_match<true>(a, text + wd.src, wd.len, [&](uint32_t j, int32_t id, uint32_t b, uint32_t e, uint32_t cb, uint32_t ce) {
                        if (j < room) {
                            row[slot + j] = id;
                            span_store(sr, slot + j, t.position + b, e - b, t.start + cb, t.start + ce, ti);
                        }
                    });
                }
            }
            at += total;
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

int launch_wordpiece(const WordpieceArgs &a, void *stream) { return launch_render(k_wordpiece_len, k_wordpiece_write<false>, a, stream); }
int launch_wordpiece_spans(const WordpieceSpanArgs &a, void *stream) { return launch_render(k_wordpiece_len, k_wordpiece_write<true>, a, stream); }

}  // namespace kgpu
