// kanpyo_amd/csrc/kgpu_spans_dev.h -- what the SPANS instantiations of the two id write kernels share (include/kanpyo_gpu.h, "ids with spans";
// kgpu_encode.hip, kgpu_wordpiece.hip): a sentence's span row, token-index row and edits, and the store of one element beside its id.  A lane that stores
// an id at row[slot] calls span_store / span_special with the same slot under the same bound: nothing here forms an address from a record's fields -- they
// are compared with edit fields and added to them (align_span, kgpu_align_core.h), and the only addresses are the sentence's edits and the two rows.
#pragma once
#include "kgpu_align_core.h"
#include "kgpu_records_dev.h"

namespace kgpu {
namespace dev {

struct SpanRow {
    kgpu_span *spans;            // element j of the sentence's sequence: spans[j] ...
    int32_t *index;              // ... and index[j]; null: no token indices were asked for
    const kgpu_norm_edit *E;     // the sentence's edits, E[0 .. ne); none without a mapping, or when the offsets run backwards
    uint64_t ne;
};
// The rows of sentence s, whose sequence starts at element `first` of the ids.
__device__ __forceinline__ SpanRow span_row(const SpanOut &o, uint64_t s, uint64_t first) {
    SpanRow r{o.spans + first, o.token_index ? o.token_index + first : nullptr, nullptr, 0};
    if (o.edits) {
        const uint64_t e0 = o.edit_offsets[s], e1 = o.edit_offsets[s + 1];
        r.E = o.edits + e0;
        r.ne = e1 > e0 ? e1 - e0 : 0;
    }
    return r;
}
// An element that comes from a record: its four fields through the edits (rules 8 to 10 of "source alignment"; no edits: as they are), ONE 16-byte store.
__device__ __forceinline__ void span_store(const SpanRow &r, uint64_t slot, uint32_t position, uint32_t byte_len, uint32_t start, uint32_t end, int32_t index) {
    const kgpu_span sp = align_span(kgpu_token{0, 0, position, start, end, byte_len}, r.E, r.ne);
    *(uint4 *)&r.spans[slot] = make_uint4(sp.position, sp.byte_len, sp.start, sp.end);
    if (r.index) r.index[slot] = index;
}
// bos, eos and pad: never mapped
__device__ __forceinline__ void span_special(const SpanRow &r, uint64_t slot) {
    *(uint4 *)&r.spans[slot] = make_uint4(0, 0, 0, 0);
    if (r.index) r.index[slot] = -1;
}

}  // namespace dev
}  // namespace kgpu
