// kanpyo_amd/csrc/kgpu_pack_rule.cpp -- kgpu_pack_host: the model inputs (include/kanpyo_gpu.h, "model inputs") on the host, the definition of what
// kgpu_pack.hip writes.  HIP-free, compiles alone (with a set_error of the caller's: tests/c_abi/pack_sanitize.cpp): pack_plan, pack_row and pack_slot
// of kgpu_pack_core.h decide every row here as they do on the device; this file adds the loops and the argument checks of rule 6.
#include "kgpu_internal.h"
#include "kgpu_pack_core.h"

int kgpu::pack_check_args(const char *who, const kgpu_pack_opts *o, uint64_t n, const void *ids_a, const void *off_a, const void *ids_b, const void *off_b,
                          uint64_t n_ids_in, const void *spans_in, const void *tix_in, const void *input_ids, const void *type_ids, const void *mask,
                          const void *spans, const void *tix, uint64_t row_capacity, const void *row_offsets, const void *status) {
    const bool pair = ids_b != nullptr || off_b != nullptr;
    if (const char *why = pack_rule_error(o, pair)) { set_error("%s: %s", who, why); return KGPU_ERR_INVALID_ARG; }
    if (!off_a || !row_offsets || (n && !status) || (pair && !off_b) || (n_ids_in && (!ids_a || (pair && !ids_b))) || (row_capacity && !input_ids)) {
        set_error("%s: null argument", who);
        return KGPU_ERR_INVALID_ARG;
    }
    if ((spans && !spans_in) || (tix && !tix_in)) { set_error("%s: spans / token indices out without spans / token indices in", who); return KGPU_ERR_INVALID_ARG; }
    const auto mis = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
    if (mis(ids_a, 4) || mis(ids_b, 4) || mis(tix_in, 4) || mis(input_ids, 4) || mis(type_ids, 4) || mis(mask, 4) || mis(tix, 4) || mis(off_a, 8) || mis(off_b, 8) ||
        mis(row_offsets, 8) || mis(spans_in, 16) || mis(spans, 16)) {
        set_error("%s: a misaligned pointer (ids, token indices, rows: 4 bytes; offsets: 8; spans: 16)", who);
        return KGPU_ERR_INVALID_ARG;
    }
    return KGPU_OK;
}

extern "C" int kgpu_pack_host(const kgpu_pack_opts *o, uint64_t n, const int32_t *ids_a, const uint64_t *off_a, const int32_t *ids_b, const uint64_t *off_b,
                              uint64_t n_ids_in, const kgpu_span *spans_in, const int32_t *tix_in, int32_t *input_ids, int32_t *type_ids, int32_t *mask,
                              kgpu_span *spans, int32_t *tix, uint64_t row_capacity, uint64_t *row_offsets, uint8_t *status, uint64_t *n_rows) {
    const char *who = "kgpu_pack_host";
    if (int rc = kgpu::pack_check_args(who, o, n, ids_a, off_a, ids_b, off_b, n_ids_in, spans_in, tix_in, input_ids, type_ids, mask, spans, tix, row_capacity,
                                       row_offsets, status))
        return rc;
    const bool pair = off_b != nullptr;
    const kgpu::PackRule r = kgpu::pack_rule(*o, pair);
    const auto plan = [&](uint64_t i) { return kgpu::pack_plan(r, off_a[i], off_a[i + 1], pair ? off_b[i] : 0, pair ? off_b[i + 1] : 0, n_ids_in); };
    // the length pass: row counts, status bytes, the scan
    uint64_t total = 0, bad_at = ~0ull;
    for (uint64_t i = 0; i < n; ++i) {
        const kgpu::PackPlan p = plan(i);
        if (p.bad && bad_at == ~0ull) bad_at = i;
        row_offsets[i] = total;
        status[i] = p.status;
        total += p.rows;
    }
    row_offsets[n] = total;
    if (n_rows) *n_rows = total;
    if (bad_at != ~0ull) {
        kgpu::set_error("%s: the input range of sample %llu runs backwards or past n_ids_in = %llu", who, (unsigned long long)bad_at, (unsigned long long)n_ids_in);
        return KGPU_ERR_INVALID_ARG;
    }
    if (total > row_capacity) {
        kgpu::set_error("%s: row buffers too small: need %llu rows, capacity %llu", who, (unsigned long long)total, (unsigned long long)row_capacity);
        return KGPU_ERR_CAPACITY;
    }
    // the write pass
    const uint64_t ML = r.max_length;
    for (uint64_t i = 0; i < n; ++i) {
        const kgpu::PackPlan p = plan(i);
        for (uint64_t k = 0; k < p.rows; ++k) {
            const kgpu::PackRow q = kgpu::pack_row(p, k);
            const uint64_t base = (row_offsets[i] + k) * ML;
            for (uint64_t j = 0; j < ML; ++j) {
                const kgpu::PackSlot s = kgpu::pack_slot(r, p, q, j);
                const bool elem = s.kind >= kgpu::PACK_SLOT_A;
                input_ids[base + j] = s.kind == kgpu::PACK_SLOT_A ? ids_a[s.src] : s.kind == kgpu::PACK_SLOT_B ? ids_b[s.src]
                                    : s.kind == kgpu::PACK_SLOT_CLS ? r.cls_id : s.kind == kgpu::PACK_SLOT_SEP ? r.sep_id : r.pad_id;
                if (type_ids) type_ids[base + j] = (int32_t)s.type;
                if (mask) mask[base + j] = s.kind != kgpu::PACK_SLOT_PAD;
                if (spans) spans[base + j] = elem ? spans_in[s.src] : kgpu_span{0, 0, 0, 0};
                if (tix) tix[base + j] = elem ? tix_in[s.src] : -1;
            }
        }
    }
    return KGPU_OK;
}
