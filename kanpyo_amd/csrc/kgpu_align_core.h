// kanpyo_amd/csrc/kgpu_align_core.h -- one token record mapped back through a line's edit records (include/kanpyo_gpu.h, "source alignment"), written
// once for the host (kgpu_normalize_table.cpp: kgpu_source_spans_host) and for the device (kgpu_align.hip): the same statements decide both.  Plain C++
// without a HIP include.  A record's fields are only ever COMPARED with edit fields and added to them (32-bit, wrapping): whatever a record holds, the
// only addresses formed are E[0 .. ne).
#pragma once
#include <cstdint>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_normalize_core.h"

namespace kgpu {

struct AlignPoint { uint32_t byte, chr; };

// How many of the line's edits E[0 .. ne) (ascending out_pos) start at or before byte v (strict: before it) of the normalised line.
template <bool STRICT>
KGPU_NORM_HD uint64_t align_edits_before(const kgpu_norm_edit *E, uint64_t ne, uint32_t v) {
    uint64_t lo = 0, hi = ne;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (STRICT ? E[mid].out_pos < v : E[mid].out_pos <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the point behind edit e, shifted by what lies between e's end and (byte, chr) in the normalised line
KGPU_NORM_HD AlignPoint align_behind(const kgpu_norm_edit &e, uint32_t byte, uint32_t chr) {
    return AlignPoint{byte - (e.out_pos + e.out_len) + (e.src_pos + e.src_len), chr - (e.out_char + e.out_chars) + (e.src_char + e.src_chars)};
}
// rule "start": where a token that starts at (byte, chr) of the normalised line starts in the source
KGPU_NORM_HD AlignPoint align_start(const kgpu_norm_edit *E, uint64_t ne, uint32_t byte, uint32_t chr) {
    const uint64_t k = align_edits_before<false>(E, ne, byte);
    if (k == 0) return AlignPoint{byte, chr};
    const kgpu_norm_edit e = E[k - 1];
    if (byte < e.out_pos + e.out_len) return AlignPoint{e.src_pos, e.src_char};   // inside the edit: the whole source segment
    return align_behind(e, byte, chr);
}
// rule "end": where a token that ends at (byte, chr) -- exclusive -- ends in the source
KGPU_NORM_HD AlignPoint align_end(const kgpu_norm_edit *E, uint64_t ne, uint32_t byte, uint32_t chr) {
    const uint64_t k = align_edits_before<true>(E, ne, byte);
    if (k == 0) return AlignPoint{byte, chr};
    const kgpu_norm_edit e = E[k - 1];
    if (byte <= e.out_pos + e.out_len) return AlignPoint{e.src_pos + e.src_len, e.src_char + e.src_chars};   // inside the edit or at its end
    return align_behind(e, byte, chr);
}
KGPU_NORM_HD kgpu_span align_span(const kgpu_token &t, const kgpu_norm_edit *E, uint64_t ne) {
    const AlignPoint a = align_start(E, ne, t.position, t.start);
    if (t.byte_len == 0) return kgpu_span{a.byte, 0u, a.chr, a.chr + (t.end - t.start)};   // the EOS dummy keeps its + 3
    const AlignPoint b = align_end(E, ne, t.position + t.byte_len, t.end);
    return kgpu_span{a.byte, b.byte - a.byte, a.chr, b.chr};
}

}  // namespace kgpu
