// kanpyo_amd/csrc/kgpu_align.hip -- the source spans of a batch's token records (include/kanpyo_gpu.h, "source alignment"): span k is token k's position,
// byte_len, start and end mapped back through its line's edit records, what kgpu_source_spans_host makes of it -- both run align_span (kgpu_align_core.h).
//
// One launch in the renders' shape (kgpu_records_dev.h: walk_sentences): one wavefront per sentence, 64 records per window, one lane per token.  A lane does
// two binary searches over its sentence's edits in global memory -- a line has few, and the lanes of a wavefront search the same ones: they come from the
// cache -- and stores its span whole, 16 bytes.  No LDS, nothing carried from window to window, no length pass: span k lies where token k lies.  A record's
// fields are compared with edit fields and added to them, never used as addresses: the only addresses formed are the sentence's edits, the record and
// its span, the last bounded by span_cap.
#include <hip/hip_runtime.h>

#include "kgpu_align_core.h"
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

__global__ __launch_bounds__(64 * RENDER_WPB) void k_source_spans(SpansArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    walk_sentences<RENDER_WPB, false>(a.b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t, const uint8_t *) {
        const uint64_t e0 = a.edit_offsets[s], e1 = a.edit_offsets[s + 1];
        const kgpu_norm_edit *E = a.edits + e0;
        const uint64_t ne = e1 > e0 ? e1 - e0 : 0;   // (offsets that run backwards: no edits)
        for (uint64_t k = k0 + lane; k < k1 && k < a.span_cap; k += 64) {
            const kgpu_span sp = align_span(a.b.tokens[k], E, ne);
            *(uint4 *)&a.spans[k] = make_uint4(sp.position, sp.byte_len, sp.start, sp.end);
        }
        return false;
    });
}

int launch_source_spans(const SpansArgs &a, void *stream) {
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.b.n + RENDER_WPB - 1) / RENDER_WPB, 8192));
    hipLaunchKernelGGL(k_source_spans, dim3((unsigned)blocks), dim3(64 * RENDER_WPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
