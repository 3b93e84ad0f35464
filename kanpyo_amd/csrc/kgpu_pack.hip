// kanpyo_amd/csrc/kgpu_pack.hip -- the model inputs of a batch's ragged ids (include/kanpyo_gpu.h, "model inputs"): padded rows [R, max_length] of
// input_ids, token_type_ids, attention_mask and, when asked for, the spans and token indices carried along.  A data-movement step: every row is decided by
// pack_plan / pack_row / pack_slot of kgpu_pack_core.h, the statements kgpu_pack_host runs, and no id is looked at.
//
// Three launches on the context's stream, the renders' shape (kgpu_records_dev.h: launch_render):
//   k_pack_len      one LANE per sample: four offsets -> its row count (closed form, windows included) and its status byte; an input range that runs
//                   backwards or past n_ids_in gives zero rows and raises the host's word [1]
//   k_lines_scan    kgpu_format.hip's, unchanged: the scan's mirror is the caller's row_offsets, the total goes to the host's word [0]
//   k_pack_write    one WAVEFRONT per output row, a grid-stride over the rows: the row's sample is the last one whose offset is <= the row (a binary search
//                   of the scanned offsets, the same words for every lane of the wavefront), its plan is made again from the four offsets, and every lane
//                   derives its slots' regions by arithmetic.  A row is a fixed amount of work whatever its sample holds: a document of eight windows keeps
//                   eight wavefronts busy, not one eight times as long.
// Loads from the ragged input are dword loads (an element's index has any parity); spans are 16-byte loads and stores, one per slot; the int32 rows are
// stored four slots to a lane as 16-byte stores when max_length is a multiple of 4 and the row arrays are 16-byte aligned (VEC), else slot by slot.
// No LDS, no atomics, no scratch.  Nothing is stored when the total exceeds row_cap, and every address is formed from a row below the total and a slot
// below max_length, or from an element index that pack_plan has range-checked against n_ids_in.
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = RENDER_WPB;

__device__ __forceinline__ PackPlan plan_of(const PackArgs &a, uint64_t i) {
    return pack_plan(a.r, a.off_a[i], a.off_a[i + 1], a.r.pair ? a.off_b[i] : 0, a.r.pair ? a.off_b[i + 1] : 0, a.n_ids_in);
}

// What slot j of a row holds, in the four int32 arrays.
struct SlotValues { int32_t id, type, mask, tix; };
__device__ __forceinline__ SlotValues slot_values(const PackArgs &a, const PackPlan &p, const PackRow &q, uint64_t j) {
    const PackSlot s = pack_slot(a.r, p, q, j);
    SlotValues v{a.r.pad_id, (int32_t)s.type, s.kind != PACK_SLOT_PAD, -1};
    if (s.kind == PACK_SLOT_A) v.id = a.ids_a[s.src];
    else if (s.kind == PACK_SLOT_B) v.id = a.ids_b[s.src];
    else if (s.kind == PACK_SLOT_CLS) v.id = a.r.cls_id;
    else if (s.kind == PACK_SLOT_SEP) v.id = a.r.sep_id;
    if (a.tix && s.kind >= PACK_SLOT_A) v.tix = a.tix_in[s.src];
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_pack_len(PackArgs a) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.b.n; i += (uint64_t)gridDim.x * 256) {
        const PackPlan p = plan_of(a, i);
        a.b.sent_len[i] = p.rows;
        a.status[i] = p.status;
        bad |= p.bad;
    }
    publish_bad(a.b, __ballot(bad) != 0);
}

template <bool VEC>
__global__ __launch_bounds__(64 * WPB) void k_pack_write(PackArgs a) {
    const uint64_t *roff = a.b.sent_len;   // the scan's offsets in device memory
    const uint64_t R = roff[a.b.n];
    if (R > a.row_cap) return;   // the host reports KGPU_ERR_CAPACITY with the rows needed
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t ML = a.r.max_length;
    for (uint64_t row = wave; row < R; row += nwaves) {
        uint64_t s = 0, hi = a.b.n;   // the last sample s in [0, n) with roff[s] <= row: samples without rows are passed over (R > 0: n > 0)
        while (hi - s > 1) {
            const uint64_t mid = s + (hi - s) / 2;
            if (roff[mid] <= row) s = mid; else hi = mid;
        }
        const PackPlan p = plan_of(a, s);
        const PackRow q = pack_row(p, row - roff[s]);
        const uint64_t base = row * ML;
        if constexpr (VEC) {
            for (uint64_t j = (uint64_t)lane * 4; j < ML; j += 256) {   // (ML is a multiple of 4: whole quads)
                const SlotValues v0 = slot_values(a, p, q, j), v1 = slot_values(a, p, q, j + 1), v2 = slot_values(a, p, q, j + 2), v3 = slot_values(a, p, q, j + 3);
                *(int4 *)&a.input_ids[base + j] = make_int4(v0.id, v1.id, v2.id, v3.id);
                if (a.type_ids) *(int4 *)&a.type_ids[base + j] = make_int4(v0.type, v1.type, v2.type, v3.type);
                if (a.mask) *(int4 *)&a.mask[base + j] = make_int4(v0.mask, v1.mask, v2.mask, v3.mask);
                if (a.tix) *(int4 *)&a.tix[base + j] = make_int4(v0.tix, v1.tix, v2.tix, v3.tix);
            }
        } else {
            for (uint64_t j = lane; j < ML; j += 64) {
                const SlotValues v = slot_values(a, p, q, j);
                a.input_ids[base + j] = v.id;
                if (a.type_ids) a.type_ids[base + j] = v.type;
                if (a.mask) a.mask[base + j] = v.mask;
                if (a.tix) a.tix[base + j] = v.tix;
            }
        }
        if (a.spans) {
            for (uint64_t j = lane; j < ML; j += 64) {   // one 16-byte load and one 16-byte store per slot, as span_store has them
                const PackSlot sl = pack_slot(a.r, p, q, j);
                uint4 sp = make_uint4(0, 0, 0, 0);
                if (sl.kind >= PACK_SLOT_A) sp = *(const uint4 *)&a.spans_in[sl.src];
                *(uint4 *)&a.spans[base + j] = sp;
            }
        }
    }
}

int launch_pack(const PackArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t len_blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.b.n + 255) / 256, 1024));
    hipLaunchKernelGGL(k_pack_len, dim3((unsigned)len_blocks), dim3(256), 0, st, a);
    launch_lines_scan(a.b, stream);
    // (the rows are counted on the device: the grid is sized by the capacity, which bounds every total that is written at all)
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.row_cap + WPB - 1) / WPB, 2048));
    const auto aligned16 = [](const void *p) { return ((uintptr_t)p & 15u) == 0; };
    const bool vec = a.r.max_length % 4 == 0 && aligned16(a.input_ids) && aligned16(a.type_ids) && aligned16(a.mask) && aligned16(a.tix);
    if (vec) hipLaunchKernelGGL(k_pack_write<true>, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    else hipLaunchKernelGGL(k_pack_write<false>, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
