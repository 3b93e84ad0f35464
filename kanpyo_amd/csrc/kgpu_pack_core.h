// kanpyo_amd/csrc/kgpu_pack_core.h -- the rule of the model inputs (include/kanpyo_gpu.h, "model inputs"), written once for the host (kgpu_pack_rule.cpp:
// kgpu_pack_host) and for the device (kgpu_pack.hip): the same statements decide both.  Plain C++ without a HIP include.  Three steps, each O(1):
//   pack_plan    a sample's four input offsets -> its trimmed ranges, its row count, its status, and the geometry every one of its rows shares
//   pack_row     row k of a planned sample -> the two slices it holds
//   pack_slot    slot j of such a row -> what stands there: a special, an element of a or b (and which one), or the pad
// Input offsets are range-checked in pack_plan (`bad`), before anything is formed from them; element values are never looked at.
#pragma once
#include <cstdint>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_normalize_core.h"   // KGPU_NORM_HD

namespace kgpu {

struct PackRule {                 // kgpu_pack_opts as the kernels take it
    uint32_t flags, strategy, max_length, stride;
    int32_t cls_id, sep_id, pad_id;
    uint32_t trim_front, trim_back;
    uint32_t pair;                // 1: the b arrays are given
};

struct PackPlan {
    uint64_t a0, La, b0, Lb;      // the trimmed sequences: ids[a0 .. a0 + La), ids[b0 .. b0 + Lb)
    uint64_t rows;
    uint64_t al, bl;              // the slice lengths of a one-row sample, and of the fixed side of a windowed one
    uint64_t w, step;             // windows: the cut side's room, and the distance between window starts
    uint8_t status;               // KGPU_PACK_OK / CUT / NO_ROOM
    uint8_t windows;              // 0: one row, slices [0, al) and [0, bl); 1: the cut side is a; 2: it is b
    bool bad;                     // an input range runs backwards or past n_ids_in (rule 8): zero rows
};

struct PackRow { uint64_t as, al, bs, bl; };   // the row holds a[as .. as + al) and b[bs .. bs + bl) of the trimmed sequences

enum : uint32_t { PACK_SLOT_PAD = 0, PACK_SLOT_CLS = 1, PACK_SLOT_SEP = 2, PACK_SLOT_A = 3, PACK_SLOT_B = 4 };
struct PackSlot { uint32_t kind; uint32_t type; uint64_t src; };   // src: the element's index in the input arrays (PACK_SLOT_A / _B only)

// rule 1: the range [o0, o1) without its trims -> first element and length
KGPU_NORM_HD void pack_trim(const PackRule &r, uint64_t o0, uint64_t o1, uint64_t &first, uint64_t &len) {
    const uint64_t raw = o1 - o0, cut = (uint64_t)r.trim_front + r.trim_back;
    len = raw > cut ? raw - cut : 0;
    first = o0 + r.trim_front;
}

KGPU_NORM_HD PackPlan pack_plan(const PackRule &r, uint64_t oa0, uint64_t oa1, uint64_t ob0, uint64_t ob1, uint64_t n_ids_in) {
    PackPlan p{0, 0, 0, 0, 0, 0, 0, 0, 0, KGPU_PACK_OK, 0, false};
    if (oa1 < oa0 || oa1 > n_ids_in || (r.pair && (ob1 < ob0 || ob1 > n_ids_in))) { p.bad = true; return p; }
    pack_trim(r, oa0, oa1, p.a0, p.La);
    if (r.pair) pack_trim(r, ob0, ob1, p.b0, p.Lb);
    const uint64_t room = r.max_length - (r.pair ? 3u : 2u);
    if (p.La <= room && p.Lb <= room - p.La) {   // rule 3 (no sum of two lengths that could wrap)
        p.rows = 1; p.al = p.La; p.bl = p.Lb;
        return p;
    }
    if (r.strategy == KGPU_PACK_LONGEST_FIRST) {   // rule 4
        p.rows = 1; p.status = KGPU_PACK_CUT;
        if (!r.pair) { p.al = room; return p; }
        uint64_t s1 = p.La <= p.Lb ? p.La : p.Lb, s2;
        if (s1 > room) s2 = s1; else s2 = s1 > room - s1 ? s1 : room - s1;
        if (s1 > room || s2 > room - s1) { s1 = room / 2; s2 = s1 + room % 2; }
        if (p.La <= p.Lb) { p.al = s1; p.bl = s2; } else { p.al = s2; p.bl = s1; }
        return p;
    }
    // rule 5: one side is fixed and kept whole, the other is cut, or cut into windows
    const bool cut_a = r.strategy == KGPU_PACK_ONLY_FIRST;
    const uint64_t fixed = cut_a ? p.Lb : p.La, L = cut_a ? p.La : p.Lb;
    const bool win = (r.flags & KGPU_PACK_WINDOWS) != 0;
    if (fixed >= room || (win && r.stride >= room - fixed)) { p.status = KGPU_PACK_NO_ROOM; return p; }   // w < 1, or no step forward
    p.w = room - fixed;
    p.status = KGPU_PACK_CUT;
    if (cut_a) { p.al = p.w; p.bl = p.Lb; } else { p.al = p.La; p.bl = p.w; }
    if (!win) { p.rows = 1; return p; }
    p.windows = cut_a ? 1 : 2;
    p.step = p.w - r.stride;
    p.rows = (L - p.w + p.step - 1) / p.step + 1;   // (L > w here: the sample did not fit.)  The last window is the first one that reaches L
    return p;
}

KGPU_NORM_HD PackRow pack_row(const PackPlan &p, uint64_t k) {
    PackRow q{0, p.al, 0, p.bl};
    if (p.windows) {
        const uint64_t L = p.windows == 1 ? p.La : p.Lb, start = k * p.step;
        const uint64_t len = L - start < p.w ? L - start : p.w;
        if (p.windows == 1) { q.as = start; q.al = len; } else { q.bs = start; q.bl = len; }
    }
    return q;
}

// rule 2
KGPU_NORM_HD PackSlot pack_slot(const PackRule &r, const PackPlan &p, const PackRow &q, uint64_t j) {
    if (j == 0) return PackSlot{PACK_SLOT_CLS, 0, 0};
    if (j <= q.al) return PackSlot{PACK_SLOT_A, 0, p.a0 + q.as + (j - 1)};
    if (j == q.al + 1) return PackSlot{PACK_SLOT_SEP, 0, 0};
    if (r.pair) {
        const uint64_t jb = j - q.al - 2;
        if (jb < q.bl) return PackSlot{PACK_SLOT_B, 1, p.b0 + q.bs + jb};
        if (jb == q.bl) return PackSlot{PACK_SLOT_SEP, 1, 0};
    }
    return PackSlot{PACK_SLOT_PAD, 0, 0};
}

// rule 6, the part that the options alone decide -> what is wrong, or null
inline const char *pack_rule_error(const kgpu_pack_opts *o, bool pair) {
    if (!o) return "null opts";
    if (o->size < sizeof(kgpu_pack_opts)) return "opts.size is smaller than the struct";
    if (o->flags & ~KGPU_PACK_WINDOWS) return "unknown flags";
    if (o->strategy > KGPU_PACK_ONLY_SECOND) return "unknown strategy";
    if (o->strategy == KGPU_PACK_LONGEST_FIRST && (o->flags & KGPU_PACK_WINDOWS)) return "KGPU_PACK_WINDOWS with KGPU_PACK_LONGEST_FIRST";
    if (o->strategy == KGPU_PACK_ONLY_SECOND && !pair) return "KGPU_PACK_ONLY_SECOND without second sequences";
    const uint32_t ns = pair ? 3 : 2;
    if (o->max_length < ns + 1 || o->max_length > 65536) return "max_length is not in ns + 1 .. 65536";
    if (o->stride >= o->max_length - ns) return "stride is not below max_length - ns";
    if (o->trim_front > 1 || o->trim_back > 1) return "trim_front / trim_back is not 0 or 1";
    return nullptr;
}
inline PackRule pack_rule(const kgpu_pack_opts &o, bool pair) {
    return PackRule{o.flags, o.strategy, o.max_length, o.stride, o.cls_id, o.sep_id, o.pad_id, o.trim_front, o.trim_back, pair ? 1u : 0u};
}

}  // namespace kgpu
