// kanpyo_amd/csrc/kgpu_words_dev.h -- device code shared by the wakati render (kgpu_words.hip), the word counts (kgpu_count.hip) and the vocabulary ids (kgpu_encode.hip): one token's
// word by the rules of include/kanpyo_gpu.h, "wakati-gaki" (field, fallback to the surface and the filter are decided per row by
// kgpu_words_host.cpp's entries; the record's range check is line_of's, kgpu_format.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kgpu_device.h"

namespace kgpu {
namespace dev {

// One token's word: len bytes at text[src] (from_text) or names[src].  kept = false: the token writes nothing (EOS, filtered out, or a bad record).
// ok = false: the record is not one the tokenizer could have written for this sentence and dictionary (line_of's rules, kgpu_format.hip).
struct Word { uint32_t len, src; bool from_text, kept, ok; };
__device__ __forceinline__ Word word_of(const WordsArgs &a, const kgpu_token &t, uint32_t B) {
    if (t.cls == KGPU_CLASS_DUMMY) return Word{0, 0, true, false, true};   // whatever its id, position and length say
    Word w{t.byte_len, t.position, true, a.drop_rowless == 0, true};
    w.ok = t.cls <= KGPU_CLASS_UNKNOWN && t.position <= B && t.byte_len <= B - t.position;
    if (t.id != 0) {
        const uint32_t id = (uint32_t)t.id, lim = t.cls == KGPU_CLASS_KNOWN ? a.n_morph : a.n_rows - a.n_morph;
        if (w.ok && t.id > 0 && id <= lim) {
            const uint2 e = *(const uint2 *)&a.rows[(t.cls == KGPU_CLASS_KNOWN ? 0u : a.n_morph) + id - 1];
            w.kept = (e.y & WORD_DROPPED) == 0;
            if ((e.y & WORD_SURFACE) == 0) { w.len = e.y & WORD_LEN_MASK; w.src = e.x; w.from_text = false; }
        } else {
            w.ok = false;
        }
    }
    if (!w.ok) w = Word{0, 0, true, false, false};
    return w;
}

// The byte-keyed tables of the word counts and the vocabulary ids (kgpu_count.hip, kgpu_encode.hip): a key's hash and the compare with an arena entry.
__device__ __forceinline__ uint32_t key_hash(const uint8_t *p, uint32_t len) {   // FNV-1a over the bytes, then murmur3's finaliser
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < len; ++i) h = (h ^ p[i]) * 16777619u;
    h ^= len;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
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

}  // namespace dev
}  // namespace kgpu
