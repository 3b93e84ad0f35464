// kanpyo_amd/csrc/kgpu_mode_core.h -- the rule of the search and extended modes (include/kanpyo_gpu.h, "search mode"), written once for the host
// (kgpu_mode_host.cpp: kgpu_mode_host) and for the device (kgpu_mode.hip): the same statements decide both.  Plain C++ without a HIP include.
//   the penalty    mode_penalty(opts, L, kanji among the L characters): what a node's word cost grows by
//   the candidate  a predecessor's dp + the target's word cost and penalty + the connection cost, int32; dropped at 1 << 30 and beyond
//   the key        one candidate (tot, pred) as ONE 64-bit word whose unsigned order is the rule's: tot ^ 0x80000000 high, pred low; all-ones = none
//   the state      a node's (dp, pre) as one 64-bit word: dp high (as it is), pre low (0xFFFFFFFF: none)
//   the record     nbest_record (kgpu_nbest_core.h), and mode_char_record for the characters of an Unknown node in extended mode
#pragma once
#include <cstdint>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_nbest_core.h"       // NBEST_INF, nbest_record
#include "kgpu_normalize_core.h"   // KGPU_NORM_HD

namespace kgpu {

constexpr uint64_t MODE_NONE = ~0ull;               // no candidate
constexpr uint32_t MODE_NO_PRE = 0xFFFFFFFFu;       // pre: None
constexpr uint64_t MODE_PENALTY_CAP = 1ull << 29;   // 2^30 + 2^29 + two int16s stays inside an int32
constexpr uint64_t MODE_MAX_NODES = 0xFFFFFFFFull;  // a node index is the low word of a key, all-ones is None

KGPU_NORM_HD bool mode_opts_valid(const kgpu_mode_opts &o) {
    return o.mode <= KGPU_MODE_EXTENDED && o.reserved[0] == 0 && o.reserved[1] == 0 && o.reserved[2] == 0;
}

// The list of include/kanpyo_gpu.h: it IS the rule.
KGPU_NORM_HD bool mode_is_kanji(uint32_t cp) {
    return cp == 0x3005u || cp == 0x3007u || (cp >= 0x3400u && cp <= 0x4DBFu) || (cp >= 0x4E00u && cp <= 0x9FFFu) || (cp >= 0xF900u && cp <= 0xFAFFu) ||
           (cp >= 0x20000u && cp <= 0x3FFFFu);
}

// The bytes of the character a lead byte opens (1 for a byte that opens none: the callers have checked the text).
KGPU_NORM_HD uint32_t mode_char_bytes(uint32_t lead) { return lead < 0x80u ? 1u : lead < 0xE0u ? 2u : lead < 0xF0u ? 3u : 4u; }
// The code point at p, in text that is UTF-8.
KGPU_NORM_HD uint32_t mode_code_point(const uint8_t *p) {
    const uint32_t b = p[0];
    if (b < 0x80u) return b;
    if (b < 0xE0u) return ((b & 0x1Fu) << 6) | (p[1] & 0x3Fu);
    if (b < 0xF0u) return ((b & 0x0Fu) << 12) | ((uint32_t)(p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu);
    return ((b & 0x07u) << 18) | ((uint32_t)(p[1] & 0x3Fu) << 12) | ((uint32_t)(p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu);
}

// The penalty of a node of L characters, `kanji` of them kanji; dummy: BOS or EOS, which get 0.  Nothing of the one-best decode is in it: N-best or
// the lattice probabilities can take it as it is.
KGPU_NORM_HD int32_t mode_penalty(const kgpu_mode_opts &o, bool dummy, uint32_t L, uint32_t kanji) {
    if (o.mode == KGPU_MODE_NORMAL || dummy) return 0;
    uint64_t p = 0;
    if (L > o.kanji_length && kanji == L) p = (uint64_t)(L - o.kanji_length) * o.kanji_penalty;
    else if (L > o.other_length) p = (uint64_t)(L - o.other_length) * o.other_penalty;
    return (int32_t)(p < MODE_PENALTY_CAP ? p : MODE_PENALTY_CAP);
}

// The candidate predecessor `pred` (its dp; BOS holds 0) -> target: its key, or MODE_NONE at 1 << 30 and beyond -- min(.., 1 << 30) then the strict '<'
// against the initial 1 << 30.  dp <= 1 << 30, word = cost + penalty <= 32767 + (1 << 29), conn an int16: the int32 sum cannot wrap.
KGPU_NORM_HD uint64_t mode_candidate(int32_t pred_dp, uint32_t pred, int32_t word, int32_t conn_cost) {
    const int32_t tot = pred_dp + word + conn_cost;
    return tot >= NBEST_INF ? MODE_NONE : (((uint64_t)((uint32_t)tot ^ 0x80000000u) << 32) | pred);
}
// The state a node keeps of its smallest key: (dp, pre), or (1 << 30, None) where nothing was accepted.
KGPU_NORM_HD uint64_t mode_state(uint64_t key) {
    return key == MODE_NONE ? (((uint64_t)(uint32_t)NBEST_INF << 32) | MODE_NO_PRE) : (key ^ (0x80000000ull << 32));
}
KGPU_NORM_HD uint64_t mode_bos_state() { return MODE_NO_PRE; }   // dp None counts 0, pre None
KGPU_NORM_HD int32_t mode_state_dp(uint64_t st) { return (int32_t)(uint32_t)(st >> 32); }
KGPU_NORM_HD uint32_t mode_state_pre(uint64_t st) { return (uint32_t)st; }

// The records a node on the chain gives: its characters for an Unknown node of more than one in extended mode, else one.
KGPU_NORM_HD uint32_t mode_record_count(uint32_t mode, uint32_t cls, uint32_t char_pos, uint32_t end_char) {
    return mode == KGPU_MODE_EXTENDED && cls == KGPU_CLASS_UNKNOWN && end_char - char_pos > 1u ? end_char - char_pos : 1u;
}
// ... and the record of character c of such a node: the bytes [byte_pos, byte_end) are that character's
KGPU_NORM_HD kgpu_token mode_char_record(int32_t id, uint32_t c, uint32_t byte_pos, uint32_t byte_end) {
    return kgpu_token{id, KGPU_CLASS_UNKNOWN, byte_pos, c, c + 1u, byte_end - byte_pos};
}

}  // namespace kgpu
