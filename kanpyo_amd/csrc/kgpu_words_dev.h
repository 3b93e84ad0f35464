// kanpyo_amd/csrc/kgpu_words_dev.h -- device code shared by the wakati render (kgpu_words.hip) and the word counts (kgpu_count.hip): one token's
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

}  // namespace dev
}  // namespace kgpu
