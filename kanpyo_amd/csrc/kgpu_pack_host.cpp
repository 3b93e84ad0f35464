// kanpyo_amd/csrc/kgpu_pack_host.cpp -- kgpu_pack_device: the model inputs (include/kanpyo_gpu.h, "model inputs"; kgpu_pack.hip) enqueued on a context, as a
// render is: the context's lines_report and lines_len, waited for by kgpu_ctx_sync_lines, which reports the rows -- KGPU_ERR_CAPACITY when they exceed
// row_capacity (nothing written), KGPU_ERR_INVALID_ARG when an input range was out of bounds.  The arguments are checked by kgpu_pack_rule.cpp, which
// kgpu_pack_host shares.
#include "kgpu_runtime.h"

extern "C" int kgpu_pack_device(kgpu_ctx *c, const kgpu_pack_opts *o, uint64_t n, const int32_t *d_ids_a, const uint64_t *d_off_a, const int32_t *d_ids_b,
                                const uint64_t *d_off_b, uint64_t n_ids_in, const kgpu_span *d_spans_in, const int32_t *d_tix_in, int32_t *d_input_ids,
                                int32_t *d_type_ids, int32_t *d_mask, kgpu_span *d_spans, int32_t *d_tix, uint64_t row_capacity, uint64_t *d_row_offsets,
                                uint8_t *d_status) {
    const char *who = "kgpu_pack_device";
    if (!c) { set_error("%s: null ctx", who); return KGPU_ERR_INVALID_ARG; }
    int rc;
    if ((rc = pack_check_args(who, o, n, d_ids_a, d_off_a, d_ids_b, d_off_b, n_ids_in, d_spans_in, d_tix_in, d_input_ids, d_type_ids, d_mask, d_spans, d_tix, row_capacity,
                              d_row_offsets, d_status)))
        return rc;
    if (row_capacity > (~0ull >> 5) / o->max_length) { set_error("%s: row_capacity x max_length does not fit an address", who); return KGPU_ERR_INVALID_ARG; }
    if ((rc = begin_records_call(c, who))) return rc;
    PackArgs a{};
    // (of the renders' batch the scan uses n, the scratch, the mirror and the host's words; there are no records and no text here)
    if ((rc = records_batch(c, DeviceRecords{nullptr, nullptr, n, nullptr, nullptr, nullptr, nullptr}, (size_t)n * 8 + 8, d_row_offsets, a.b))) return rc;
    a.r = pack_rule(*o, d_off_b != nullptr);
    a.ids_a = d_ids_a; a.ids_b = d_ids_b; a.off_a = d_off_a; a.off_b = d_off_b; a.n_ids_in = n_ids_in;
    a.spans_in = d_spans_in; a.tix_in = d_tix_in;
    a.input_ids = d_input_ids; a.type_ids = d_type_ids; a.mask = d_mask; a.tix = d_tix; a.spans = d_spans;
    a.row_cap = row_capacity; a.status = d_status;
    if ((rc = records_launched(c, launch_pack(a, c->stream), who, "pack", row_capacity))) return rc;
    c->lines_report.bad_what = "kgpu_pack_device: an input range runs backwards or past n_ids_in";
    return KGPU_OK;
}
