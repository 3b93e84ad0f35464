// kanpyo_amd/csrc/kgpu_records_dev.h -- device code shared by the consumers of a batch's 24-byte records, one sentence per wavefront: the `kanpyo tokenize`
// lines (kgpu_format.hip), the wakati lines (kgpu_words.hip), the vocabulary ids (kgpu_encode.hip) and the word counts (kgpu_count.hip).  Written once, here:
//   record_of        the rules a record must keep to be one the tokenizer could have written for its sentence and dictionary, and its feature row
//   word_of          one token's word by the rules of include/kanpyo_gpu.h, "wakati-gaki" (field, fallback to the surface and the filter are decided per
//                    row by kgpu_words_host.cpp's entries); row_determined: the words that one feature row names
//   walk_sentences   the grid-stride over sentences of every kernel: token range, byte length, text, the bad-record flag, the status mirror
//   sentence_units   the first of a render's three launches: a sentence's units (bytes, ids) summed -> sent_len[s]; records are range-checked here
//   write_units      the heart of a text render's third launch: a window of pieces whose starts lie in LDS, assembled into aligned 16-byte units
//   launch_render    the three launches on a stream: lengths, k_lines_scan (kgpu_format.hip: exclusive scan of sent_len in place, mirrored into the
//                    caller's offsets, the total published to the host's mapped words), write
//   key_hash, entry_equals, table_lookup   the byte-keyed tables of the counts and the ids
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "kgpu_device.h"

namespace kgpu {
namespace dev {

constexpr uint32_t RENDER_WPB = 4;   // wavefronts per workgroup of the renders (one sentence each at a time)

// ok = false: the record is not one the tokenizer could have written for this sentence and dictionary: a class above UNKNOWN, a surface that leaves the
// sentence's B bytes, an id that is negative or above the class's rows.  The dummy class (EOS) is exempt, whatever its id, position and length say.
// has_row: the token has a feature row (id 0 -- BOS_EOS_ID, src/lattice/node.rs:3 -- has none), and `row` is it.
struct Record { bool ok, has_row; uint32_t row; };
__device__ __forceinline__ Record record_of(const RecordsBatch &b, const kgpu_token &t, uint32_t B) {
    if (t.cls == KGPU_CLASS_DUMMY) return Record{true, false, 0};
    Record r{t.cls <= KGPU_CLASS_UNKNOWN && t.position <= B && t.byte_len <= B - t.position, false, 0};
    if (t.id != 0) {
        const bool known = t.cls == KGPU_CLASS_KNOWN;
        r.ok = r.ok && t.id > 0 && (uint32_t)t.id <= (known ? b.n_morph : b.n_rows - b.n_morph);
        r.has_row = r.ok;
        r.row = feature_row(known, b.n_morph, (uint32_t)t.id);
    }
    return r;
}

// One token's word: len bytes at text[src] (from_text) or names[src].  kept = false: the token writes nothing (EOS, filtered out, or a bad record).
struct Word { uint32_t len, src; bool from_text, kept, ok; };
__device__ __forceinline__ Word word_of(const RecordsBatch &b, const WordTable &wt, const kgpu_token &t, uint32_t B) {
    const Record r = record_of(b, t, B);
    if (!r.ok || t.cls == KGPU_CLASS_DUMMY) return Word{0, 0, true, false, r.ok};
    Word w{t.byte_len, t.position, true, wt.drop_rowless == 0, true};
    if (r.has_row) {
        const uint2 e = *(const uint2 *)&wt.rows[r.row];
        w.kept = (e.y & WORD_DROPPED) == 0;
        if ((e.y & WORD_SURFACE) == 0) { w.len = e.y & WORD_LEN_MASK; w.src = e.x; w.from_text = false; }
    }
    return w;
}
// Is a kept word named by its token's feature row alone (a known token with a row; a pool name), or by its bytes in the text?  (word_of has checked the id.)
__device__ __forceinline__ bool row_determined(const kgpu_token &t, const Word &w) { return t.id != 0 && (t.cls == KGPU_CLASS_KNOWN || !w.from_text); }

// The walk of WPB-wavefront workgroups over a batch: wavefront by wavefront the sentences s, s + (wavefronts of the grid), ...  For each one the wavefront
// calls body(s, k0, k1, B, text) -- its records are tokens[k0 .. k1) (none when the offsets run backwards: a bad record), its text is text[0 .. B) -- which
// returns whether this lane met a bad record.  MIRROR: lane 0 copies the sentence's status byte to the caller.  -> (wave-uniform) a bad record anywhere.
template <uint32_t WPB, bool MIRROR, class Body>
__device__ __forceinline__ bool walk_sentences(const RecordsBatch &b, Body &&body) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    bool bad = false;
    for (uint64_t s = wave; s < b.n; s += nwaves) {
        const uint64_t k0 = b.tok_offsets[s], k1 = b.tok_offsets[s + 1];
        const uint32_t B = (uint32_t)(b.offsets[s + 1] - b.offsets[s]);
        bad |= k1 < k0;
        if (MIRROR && lane == 0 && b.status_out) b.status_out[s] = b.status_in[s];
        bad |= body(s, k0, k1, B, b.utf8 + b.offsets[s]);
    }
    return __ballot(bad) != 0;
}
// ... as the renders publish it: straight to the host's word
__device__ __forceinline__ void publish_bad(const RecordsBatch &b, bool anybad) {
    if (anybad && (threadIdx.x & 63) == 0) __hip_atomic_store(&b.host_ctl[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A length kernel's body.  units(token, B) -> what the token contributes and whether its record is good -- or units(token, B, text) where the units depend on
// the sentence's bytes (kgpu_wordpiece.hip); stored(sum) -> the sentence's entry of sent_len.
struct Units { uint64_t n; bool ok; };
template <class U, class S>
__device__ __forceinline__ void sentence_units(const RecordsBatch &b, U &&units, S &&stored) {
    const uint32_t lane = threadIdx.x & 63;
    publish_bad(b, walk_sentences<RENDER_WPB, true>(b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        uint64_t sum = 0;
        bool bad = false;
        for (uint64_t k = k0 + lane; k < k1; k += 64) {
            Units u;
            if constexpr (std::is_invocable_v<U, const kgpu_token &, uint32_t, const uint8_t *>) u = units(b.tokens[k], B, text);
            else u = units(b.tokens[k], B);
            sum += u.n;
            bad |= !u.ok;
        }
        sum = wave_sum64(sum);
        if (lane == 0) b.sent_len[s] = stored(sum);
        return bad;
    }));
}

// One window of a sentence's text: mk pieces (mk >= 1, every piece a byte at least) whose starts, relative to the sentence's first output byte, are
// st[0 .. mk) in the wavefront's LDS row; together they are the output bytes [T0 + base, T0 + wend).  16-byte units are aligned in the address space:
// output byte p lives at unit (p + mis) / 16 of abase = text - mis.  Every lane assembles one unit at a time and stores it whole; only the units a window
// shares with its neighbours (a sentence's head and tail, and the ends of the caller's buffer) are stored byte by byte.  `last`: the sentence's last byte.
// The policy P says what a piece is:  P::Piece p.load(j) -- piece j's fields from LDS;  p.length(piece);  p.byte(piece, rel, is_last) -- its byte `rel`.
template <class P>
__device__ __forceinline__ void write_units(uint8_t *abase, uint64_t mis, uint64_t T0, uint64_t base, uint64_t wend, uint64_t last, const uint64_t *st,
                                            uint32_t mk, const P &p) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t lo = T0 + base + mis, hi = T0 + wend + mis;
    for (uint64_t u = lo / 16 + lane; u * 16 < hi; u += 64) {
        const uint64_t q0 = u * 16 > lo ? u * 16 : lo, q1 = u * 16 + 16 < hi ? u * 16 + 16 : hi;
        const uint64_t r0 = q0 - mis - T0;   // sentence-relative offset of the unit's first byte of ours
        uint32_t j = 0;                      // the piece holding it: the last j with st[j] <= r0
        for (uint32_t step = 32; step > 0; step >>= 1)
            if (j + step < mk && st[j + step] <= r0) j += step;
        uint64_t ps = st[j];
        typename P::Piece pc = p.load(j);
        uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t b = 0; b < 16; ++b) {
            const uint64_t q = u * 16 + b;
            if (q < q0 || q >= q1) continue;
            const uint64_t r = q - mis - T0;
            uint64_t rel = r - ps;
            if (rel >= p.length(pc)) {   // the next piece starts here
                ++j;
                ps = st[j]; pc = p.load(j);
                rel = r - ps;
            }
            word[b >> 2] |= p.byte(pc, rel, r == last) << (8 * (b & 3));
        }
        if (q0 == u * 16 && q1 == u * 16 + 16) {
            *(uint4 *)(abase + u * 16) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {   // a unit shared with the neighbouring window, sentence or the bytes outside the buffer: ours only
            for (uint64_t q = q0; q < q1; ++q) abase[q] = (uint8_t)(word[(q & 15) >> 2] >> (8 * (q & 3)));
        }
    }
}

// A render's three launches on a stream.  -> hipGetLastError()
// (A write kernel whose arguments DERIVE from the length kernel's -- the span instantiations of the ids -- gives the length kernel its base part.)
template <class LenArgs, class Args>
int launch_render(void (*len)(LenArgs), void (*write)(Args), const Args &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.b.n + RENDER_WPB - 1) / RENDER_WPB, 8192));
    hipLaunchKernelGGL(len, dim3((unsigned)blocks), dim3(64 * RENDER_WPB), 0, st, static_cast<const LenArgs &>(a));
    launch_lines_scan(a.b, stream);
    hipLaunchKernelGGL(write, dim3((unsigned)blocks), dim3(64 * RENDER_WPB), 0, st, a);
    return (int)hipGetLastError();
}

// The byte-keyed tables of the word counts and the vocabulary ids (kgpu_count.hip, kgpu_encode.hip): a key's hash and the compare with an arena entry.
// key_hash = key_hash_finish(state after the bytes, length): a consumer that walks a word forward once (kgpu_wordpiece.hip) carries the state and finishes
// it at every prefix it probes.  The value is what the host computes (vocab_key_hash, kgpu_vocab_table.cpp).
constexpr uint32_t KEY_HASH_INIT = 2166136261u;
__device__ __forceinline__ uint32_t key_hash_step(uint32_t state, uint32_t byte) { return (state ^ byte) * 16777619u; }   // FNV-1a
__device__ __forceinline__ uint32_t key_hash_finish(uint32_t h, uint32_t len) {   // the length folded in, then murmur3's finaliser
    h ^= len;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t key_hash(const uint8_t *p, uint32_t len) {   // FNV-1a over the bytes, then murmur3's finaliser
    uint32_t h = KEY_HASH_INIT;
    for (uint32_t i = 0; i < len; ++i) h = key_hash_step(h, p[i]);
    return key_hash_finish(h, len);
}

// Does the arena entry at e hold exactly these bytes?  (The entry is padded to 8 bytes: whole words are read from it, single bytes from the text.)
__device__ __forceinline__ bool entry_equals(const uint8_t *e, uint32_t h, const uint8_t *p, uint32_t len) {
    const uint2 head = *(const uint2 *)e;
    if (head.x != len || head.y != h) return false;
    for (uint32_t i = 0; i < len; i += 8) {
        const unsigned long long v = *(const unsigned long long *)(e + COUNT_ENTRY_HEAD + i);
        const uint32_t m = len - i < 8 ? len - i : 8;
        for (uint32_t b = 0; b < m; ++b)
            if ((uint32_t)((v >> (8 * b)) & 0xFFu) != p[i + b]) return false;
    }
    return true;
}

// A READ-ONLY probe of a frozen table of {tag, id} slots (kgpu_vocab_table.cpp; T: anything with `slots`, `slot_mask` and `arena` -- EncodeArgs, ByteTable): the
// id of the len bytes at p, whose hash is h -- the slot whose tag carries the hash and whose arena entry holds the same length and bytes; a free slot ends
// the probe -- or `none`.  Plain loads, bounded by the table.
template <class T>
__device__ __forceinline__ int32_t table_lookup(const T &a, uint32_t h, const uint8_t *p, uint32_t len, int32_t none) {
    uint32_t i = h & a.slot_mask;
    for (uint64_t probes = 0; probes <= a.slot_mask; ++probes, i = (i + 1) & a.slot_mask) {   // (64-bit: bounded at 2^32 slots too)
        const uint4 sl = *(const uint4 *)&a.slots[i];   // tag (x, y), id (z)
        if ((sl.x | sl.y) == 0) break;
        if (sl.y == h && entry_equals(a.arena + ((uint64_t)sl.x - 1) * 8, h, p, len)) return (int32_t)sl.z;
    }
    return none;
}

}  // namespace dev
}  // namespace kgpu
