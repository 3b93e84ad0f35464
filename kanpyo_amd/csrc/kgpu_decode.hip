// kanpyo_amd/csrc/kgpu_decode.hip -- the text from ids on the device (include/kanpyo_gpu.h, "text from ids"; not an output of the reference): for every
// sequence of ids ONE line, the words of its kept elements joined by the rule of kgpu_decode_core.h -- which kgpu_decode_host.cpp runs on the host:
// the same statements decide both.  No terminator: a sequence without a byte writes nothing.
//
// Three launches on the context's stream (kgpu_records_dev.h: launch_render):
//   k_decode_len    one wavefront per sequence, 64 ids at a time (consecutive dwords): every lane classifies its id (skip list, range), loads its
//                   entry's length and first eight bytes (one load: an entry's bytes are padded to 8) and takes its piece; whether it is kept
//                   element 0 is a ballot and a prefix count inside the window and a wave-uniform carry across windows.  The line's bytes (a 64-bit
//                   wave sum) go to sent_len[s], the status bit (a ballot) to status[s].
//   k_lines_scan    kgpu_format.hip's
//   k_decode_write  the same walk: the pieces that hold a byte at least are compacted (ballot + prefix count) into LDS with their starts (a wave scan)
//                   and handed to write_units.  A piece is its separator bytes, then the word's bytes from the arena behind the stripped prefix.
// No lane loops over a word: bytes are produced by write_units' unit-parallel loop.  Plain loads and stores only.
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = RENDER_WPB;

// One element as both passes see it: rule 1's answer, and for a kept one its piece and where its word's bytes lie in the arena.
struct Elem { bool kept, bad; DecodePiece p; uint32_t e; };
// seen: a kept element stands in front of this window; -> the lane's element, and in `keep` the window's kept lanes.
__device__ __forceinline__ Elem elem_of(const DecodeArgs &a, uint64_t k, bool in_window, bool seen, uint32_t lane, unsigned long long &keep) {
    Elem el{false, false, DecodePiece{0, 0, 0}, 0};
    int32_t id = 0;
    if (in_window) {
        id = a.ids[k];
        const DecodeClass c = decode_class(a.r, id);
        el.kept = c.kept; el.bad = c.bad;
    }
    keep = __ballot(el.kept);
    if (el.kept) {
        el.e = a.entry[(uint32_t)id];
        const uint8_t *ent = a.arena + (uint64_t)el.e * 8;
        const uint32_t len = *(const uint32_t *)ent;
        const uint64_t head = *(const unsigned long long *)(ent + COUNT_ENTRY_HEAD);   // (inside the arena whatever the length: its spare bytes)
        const bool first = !seen && (keep & ((1ull << lane) - 1)) == 0;
        el.p = decode_piece(a.r, first, len, head);
    }
    return el;
}

// The grid-stride over sequences of both kernels: wavefront by wavefront the sequences s, s + (wavefronts of the grid), ...; body(s, k0, k1): its ids
// are ids[k0 .. k1) (none when the offsets run backwards).
template <class Body>
__device__ __forceinline__ void walk_sequences(const DecodeArgs &a, Body &&body) {
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    for (uint64_t s = wave; s < a.b.n; s += nwaves) {
        const uint64_t k0 = a.id_offsets ? a.id_offsets[s] : s * a.width;
        const uint64_t k1 = a.id_offsets ? a.id_offsets[s + 1] : (s + 1) * a.width;
        body(s, k0, k1 < k0 ? k0 : k1);
    }
}

// write_units' pieces: fields in the wavefront's LDS rows
struct DecodePieces {
    const uint32_t *ent, *len, *ss;   // the arena entry (8-byte units), the word bytes taken, separator bytes | skipped bytes << 8
    const uint8_t *arena;
    uint64_t sep;
    struct Piece { uint32_t ent, len, ss; };
    __device__ __forceinline__ Piece load(uint32_t j) const { return Piece{ent[j], len[j], ss[j]}; }
    __device__ __forceinline__ uint64_t length(const Piece &p) const { return (uint64_t)(p.ss & 0xFFu) + p.len; }
    __device__ __forceinline__ uint32_t byte(const Piece &p, uint64_t rel, bool) const {
        const uint32_t ns = p.ss & 0xFFu;
        if (rel < ns) return (uint32_t)(sep >> (8 * rel)) & 0xFFu;
        return arena[(uint64_t)p.ent * 8 + COUNT_ENTRY_HEAD + (p.ss >> 8) + (rel - ns)];
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_decode_len(DecodeArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    walk_sequences(a, [&](uint64_t s, uint64_t k0, uint64_t k1) {
        uint64_t sum = 0;
        bool seen = false, bad = false;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            unsigned long long keep;
            const Elem el = elem_of(a, kw + lane, lane < k1 - kw, seen, lane, keep);
            sum += el.kept ? el.p.bytes() : 0;
            bad |= el.bad;
            seen = seen || keep != 0;
        }
        sum = wave_sum64(sum);
        const bool anybad = __ballot(bad) != 0;
        if (lane == 0) { a.b.sent_len[s] = sum; a.status[s] = anybad ? KGPU_DECODE_BAD_ID : KGPU_DECODE_OK; }
    });
}

__global__ __launch_bounds__(256) void k_decode_write(DecodeArgs a) {
    __shared__ uint64_t st_s[WPB][64];                                  // piece start, relative to the line's first byte
    __shared__ uint32_t ent_s[WPB][64], len_s[WPB][64], ss_s[WPB][64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t *toff = a.b.sent_len;    // the scan's offsets in device memory
    if (toff[a.b.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    uint8_t *const abase = a.text - mis;
    uint64_t *st = st_s[w];
    uint32_t *ent = ent_s[w], *len = len_s[w], *ss = ss_s[w];
    walk_sequences(a, [&](uint64_t s, uint64_t k0, uint64_t k1) {
        const uint64_t T0 = toff[s];
        uint64_t base = 0;
        bool seen = false;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            unsigned long long keep;
            const Elem el = elem_of(a, kw + lane, lane < k1 - kw, seen, lane, keep);
            seen = seen || keep != 0;
            const uint64_t n = el.kept ? el.p.bytes() : 0;
            const unsigned long long full = __ballot(n != 0);   // the pieces write_units may search: a byte at least each
            if (full == 0) continue;   // (wave-uniform) a window without a byte writes nothing
            const uint32_t mk = (uint32_t)__popcll(full), rank = (uint32_t)__popcll(full & ((1ull << lane) - 1));
            const uint64_t incl = wave_incl_scan64(n, lane);
            const uint64_t wend = base + lane63(incl);
            wave_sync();   // the previous window's readers are through
            if (n != 0) { st[rank] = base + incl - n; ent[rank] = el.e; len[rank] = el.p.len; ss[rank] = el.p.sep | (el.p.skip << 8); }
            wave_sync();
            write_units(abase, mis, T0, base, wend, ~0ull /* no terminator: a `last` no byte reaches */, st, mk, DecodePieces{ent, len, ss, a.arena, a.r.sep});
            base = wend;
        }
    });
}

int launch_decode(const DecodeArgs &a, void *stream) { return launch_render(k_decode_len, k_decode_write, a, stream); }

}  // namespace kgpu
