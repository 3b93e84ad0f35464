// kanpyo_amd/csrc/kgpu_normalize.hip -- NFC / NFKC of a batch of lines in HBM (include/kanpyo_gpu.h, "text normalisation"): line i of the output is
// the normalisation of line i of the input, byte for byte what kgpu_normalize_host makes of it -- both run norm_segment (kgpu_normalize_core.h).
//
// A line is cut into SEGMENTS at its boundaries (a property of single code points: the header states it), and a segment's result depends on nothing outside
// it, so every segment is some lane's own work.  One wavefront per line, 1024 bytes of the ADDRESS space per pass, one aligned 16-byte unit per lane:
// the lane decodes the code points that START in its unit (and the one behind them, for its boundary bit), looks their property words up and knows
//   - which of them start a segment (a boundary, or the line's first code point),
//   - which of those segments are a single inert code point followed by a boundary or the line's end: they are copied, which is nearly all of Japanese text,
//   - and walks the others itself, reading on past its unit: decompose, reorder, compose in its own column of a 65-entry LDS buffer
//     (a runtime-indexed private array would live in scratch memory).
// Three launches on the context's stream, a fixed number whatever the batch holds, no host round trip between them, no workgroup waits for another:
//   k_norm_len    per line: UTF-8 checked, the output length (the line's own when it is not UTF-8 or a segment is oversize), the status byte, and how
//                 the write pass treats the line (MODE_COPY: it comes out as it went in)
//   k_lines_scan  (kgpu_format.hip) exclusive scan into the caller's text_offsets; the total to the host's mapped words
//   k_norm_write  the same walk with a wavefront prefix sum of the lanes' output bytes; MODE_COPY lines are copied in 16-byte units where source and
//                 destination are aligned alike.  Nothing is written when the total exceeds the capacity.
// Walked segments are normalised three times in all (once for the length, twice in the write pass: its size, then its bytes) and their bytes are stored
// one by one: the price of keeping nothing between the launches but a length per line.  Clean text never pays it.
//
// Both kernels are templates on ALIGN.  <false> is the normaliser above, statement for statement.  <true> (include/kanpyo_gpu.h, "source alignment") also
// keeps what the write pass knows at the moment it stores a segment -- where it starts and ends in the source and in the output -- as one 24-byte edit
// record per walked segment whose bytes changed (norm_segment_edit, kgpu_normalize_core.h: the host's statements):
//   k_norm_len<true>    also counts each line's edits; a second k_lines_scan turns the counts into the caller's edit_offsets (four launches in all)
//   k_norm_write<true>  three more wavefront prefix sums per pass beside the byte scan -- edits emitted, output code points, source code points (the
//                       popcount of classify's lead mask) -- and their totals carried from pass to pass; a lane stores its edits with plain stores,
//                       each bounded by the line's scanned edit count as the text stores are bounded by its length
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kgpu_device.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t PASS = 1024;          // bytes of the address space per wavefront pass: 64 lanes x 16
constexpr uint32_t MODE_NORMALIZE = 0, MODE_COPY = 1;

// a lane's column of the wavefront's segment buffer: entry i at seg[i * 64 + lane] (the lanes of a wavefront hit 64 different banks)
struct LdsColumn {
    uint32_t *col;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return col[i * 64]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) { col[i * 64] = v; }
};

// Four aligned bytes at position q of the line (q + the line's address is a multiple of 4), zero where the line has none.
__device__ __forceinline__ uint32_t load_word(const uint8_t *line, int64_t q, int64_t len) {
    if (q >= 0 && q + 4 <= len) return *(const uint32_t *)(line + q);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (q + b >= 0 && q + b < len) v |= (uint32_t)line[q + b] << (8 * b);
    return v;
}

// What a lane knows about its unit, as bit masks over the unit's bytes 0 .. 15 and the four behind them (bits 16 .. 19): a code point starts there
// (lead), has a boundary before it (bnd), is inert (inert).  bad: a byte of the unit belongs to no valid sequence.
struct Masks { uint32_t lead, bnd, inert; bool bad; };

// The sequence whose bytes are t (lowest byte first; zero behind the line's end): norm_decode on registers.
__device__ __forceinline__ uint32_t decode4(uint32_t t, bool &ok) {
    const uint32_t b = t & 0xFFu, b1 = (t >> 8) & 0xFFu, b2 = (t >> 16) & 0xFFu, b3 = t >> 24;
    const bool c1 = (b1 & 0xC0u) == 0x80u, c2 = (b2 & 0xC0u) == 0x80u, c3 = (b3 & 0xC0u) == 0x80u;
    uint32_t cp;
    if (b < 0x80) { ok = true; return b; }
    if (b >= 0xC2 && b <= 0xDF) { ok = c1; cp = (b & 0x1Fu) << 6 | (b1 & 0x3Fu); }
    else if ((b & 0xF0u) == 0xE0u) { cp = (b & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu); ok = c1 && c2 && cp >= 0x800 && !(cp >= 0xD800 && cp <= 0xDFFF); }
    else if (b >= 0xF0 && b <= 0xF4) { cp = (b & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu); ok = c1 && c2 && c3 && cp >= 0x10000 && cp <= 0x10FFFF; }
    else { ok = false; cp = 0; }
    return ok ? cp : 0xFFFDu;
}
// bytes a lead byte announces (0: no lead byte)
__device__ __forceinline__ uint32_t lead_len(uint32_t b) { return b < 0x80 ? 1u : (b >= 0xC2 && b <= 0xDF) ? 2u : (b & 0xF0u) == 0xE0u ? 3u : (b >= 0xF0 && b <= 0xF4) ? 4u : 0u; }

// r0: the unit's position in the line (negative in front of a line that does not start at a 16-byte boundary)
__device__ __forceinline__ Masks classify(const NormTables &t, uint32_t form, const uint8_t *line, int64_t len, int64_t r0) {
    uint32_t W[7];   // bytes r0 - 4 .. r0 + 24 (every index below is a compile-time constant: the array stays in registers)
    if (r0 >= 0 && r0 + 16 <= len) {
        const uint4 v = *(const uint4 *)(line + r0);
        W[1] = v.x; W[2] = v.y; W[3] = v.z; W[4] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) W[1 + k] = load_word(line, r0 + 4 * k, len);
    }
    W[0] = load_word(line, r0 - 4, len);
    W[5] = load_word(line, r0 + 16, len);
    W[6] = load_word(line, r0 + 20, len);
    Masks m{0, 0, 0, false};
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        const int64_t pos = r0 + k;
        if (pos < 0 || pos >= len) continue;
        const uint32_t tt = __funnelshift_r(W[1 + (k >> 2)], W[2 + (k >> 2)], 8 * (k & 3));
        const uint32_t b = tt & 0xFFu;
        if ((b & 0xC0u) == 0x80u) {   // a continuation byte: the nearest byte in front of it that is none must announce a sequence that reaches it
            if (k < 16) {
                const uint32_t tb = __funnelshift_r(W[(k + 1) >> 2], W[((k + 1) >> 2) + 1], 8 * ((k + 1) & 3));   // bytes k - 3 .. k (zero in front of the line)
                const uint32_t p1 = (tb >> 16) & 0xFFu, p2 = (tb >> 8) & 0xFFu, p3 = tb & 0xFFu;
                const bool n1 = (p1 & 0xC0u) != 0x80u, n2 = (p2 & 0xC0u) != 0x80u;
                const bool covered = n1 ? lead_len(p1) >= 2 : n2 ? lead_len(p2) >= 3 : lead_len(p3) == 4;
                if (!covered) m.bad = true;
            }
            continue;
        }
        bool ok;
        const uint32_t cp = decode4(tt, ok);
        if (!ok && k < 16) m.bad = true;
        const uint32_t w = norm_props(t, cp);
        m.lead |= 1u << k;
        m.bnd |= (uint32_t)norm_boundary(w, form) << k;
        m.inert |= (uint32_t)norm_inert(w, form) << k;
    }
    return m;
}

// The segments that start in a lane's unit, in order.  single(k, l): a single inert code point of l bytes at byte k of the unit; walk(k): any other.
template <class Single, class Walk>
__device__ __forceinline__ void each_segment(const Masks &m, int64_t len, int64_t r0, Single &&single, Walk &&walk) {
    uint32_t starts = m.lead & m.bnd & 0xFFFFu;
    if (r0 <= 0 && r0 > -16) starts |= m.lead & (1u << (uint32_t)(-r0));   // the line's first code point starts a segment whatever it is
    for (; starts; starts &= starts - 1) {
        const uint32_t k = (uint32_t)__builtin_ctz(starts);
        const uint32_t above = m.lead >> (k + 1);
        const uint32_t nx = above ? k + 1 + (uint32_t)__builtin_ctz(above) : 32u;   // where the next code point starts (none: the line ends)
        if (((m.inert >> k) & 1u) && (!above || ((m.bnd >> nx) & 1u))) single(k, above ? nx - k : (uint32_t)(len - (r0 + k)));
        else walk(k);
    }
}

struct Line { const uint8_t *p; uint64_t len; uint32_t mis; };
__device__ __forceinline__ Line line_of(const NormArgs &a, uint64_t i) {
    const uint64_t lo = a.offsets[i], hi = a.offsets[i + 1];
    const uint8_t *p = a.utf8 + lo;
    return Line{p, hi - lo, (uint32_t)((uintptr_t)p & 15u)};
}

template <bool ALIGN> using ArgsOf = std::conditional_t<ALIGN, NormAlignArgs, NormArgs>;

}  // namespace

template <bool ALIGN>
__global__ __launch_bounds__(64) void k_norm_len(ArgsOf<ALIGN> a) {
    __shared__ uint32_t seg[NORM_BUF * 64];
    const uint32_t lane = threadIdx.x;
    LdsColumn buf{seg + lane};
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const Line L = line_of(a, i);
        if (L.len >= (1ull << 32)) {   // (positions inside a line are 32-bit)
            if (lane == 0) {
                a.sent_len[i] = L.len; a.mode[i] = MODE_COPY; a.status[i] = KGPU_SENT_NOT_NORMALIZED;
                if constexpr (ALIGN) a.edit_len[i] = 0;
            }
            continue;
        }
        const int64_t len = (int64_t)L.len;
        const uint32_t end = (uint32_t)L.len;
        uint64_t bytes = 0;
        uint32_t edits = 0;   // (ALIGN) walked segments of this lane whose bytes change
        bool bad = false, over = false, walked = false;
        for (int64_t u = 0; u < (int64_t)L.mis + len; u += PASS) {
            const int64_t r0 = u + lane * 16 - (int64_t)L.mis;
            if (r0 + 16 <= 0 || r0 >= len) continue;
            const Masks m = classify(a.t, a.form, L.p, len, r0);
            bad |= m.bad;
            each_segment(m, len, r0, [&](uint32_t, uint32_t l) { bytes += l; },
                         [&](uint32_t k) {
                             uint32_t n, next;
                             const uint32_t r = norm_segment(a.t, a.form, L.p, (uint32_t)(r0 + k), end, buf, n, next);
                             walked = true;
                             if (r == NORM_OVERSIZE) over = true;
                             else {
                                 bytes += r;
                                 if constexpr (ALIGN) edits += norm_segment_edit(L.p, (uint32_t)(r0 + k), next, buf, n, r).differs;
                             }
                         });
        }
        const bool any_bad = __ballot(bad) != 0, any_over = __ballot(over) != 0, any_walked = __ballot(walked) != 0;
        const uint64_t total = wave_sum64(bytes);
        if (lane == 0) {
            const bool as_it_is = any_bad || any_over;
            a.sent_len[i] = as_it_is ? L.len : total;
            a.mode[i] = (as_it_is || !any_walked) ? MODE_COPY : MODE_NORMALIZE;
            a.status[i] = any_bad ? KGPU_SENT_INVALID_UTF8 : any_over ? KGPU_SENT_NOT_NORMALIZED : KGPU_SENT_OK;
        }
        if constexpr (ALIGN) {   // (a line that comes out as it went in has no edits)
            const uint32_t line_edits = wave_sum(edits);
            if (lane == 0) a.edit_len[i] = (any_bad || any_over) ? 0u : line_edits;
        }
    }
}

template <bool ALIGN>
__global__ __launch_bounds__(64) void k_norm_write(ArgsOf<ALIGN> a) {
    __shared__ uint32_t seg[NORM_BUF * 64];
    const uint64_t *toff = a.sent_len;   // the scan's offsets in device memory
    if (toff[a.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint64_t *eoff = nullptr;       // (ALIGN) ... and the edits'
    if constexpr (ALIGN) {
        eoff = a.edit_len;
        if (eoff[a.n] > a.edit_cap) return;   // either size may be the one that does not fit: nothing is written then
    }
    const uint32_t lane = threadIdx.x;
    LdsColumn buf{seg + lane};
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const Line L = line_of(a, i);
        uint8_t *dst = a.text + toff[i];
        const uint64_t out_len = toff[i + 1] - toff[i];
        if (a.mode[i] == MODE_COPY) {   // as it is: 16-byte units where the two addresses are aligned alike, else words, else bytes
            const uint64_t n = L.len < out_len ? L.len : out_len;   // (equal, unless the batch changed under the launches)
            const uint32_t dmis = (uint32_t)((uintptr_t)dst & 15u);
            if (dmis == L.mis) {
                const uint64_t to_boundary = (16u - dmis) & 15u, head = to_boundary < n ? to_boundary : n, nfull = (n - head) / 16;
                if (lane < head) dst[lane] = L.p[lane];
                for (uint64_t j = lane; j < nfull; j += 64) *(uint4 *)(dst + head + 16 * j) = *(const uint4 *)(L.p + head + 16 * j);
                const uint64_t tail = head + 16 * nfull;
                if (tail + lane < n) dst[tail + lane] = L.p[tail + lane];
            } else if (((dmis ^ L.mis) & 3u) == 0) {
                const uint64_t to_boundary = (4u - (dmis & 3u)) & 3u, head = to_boundary < n ? to_boundary : n, nfull = (n - head) / 4;
                if (lane < head) dst[lane] = L.p[lane];
                for (uint64_t j = lane; j < nfull; j += 64) *(uint32_t *)(dst + head + 4 * j) = *(const uint32_t *)(L.p + head + 4 * j);
                const uint64_t tail = head + 4 * nfull;
                if (tail + lane < n) dst[tail + lane] = L.p[tail + lane];
            } else {
                for (uint64_t j = lane; j < n; j += 64) dst[j] = L.p[j];
            }
            continue;
        }
        const int64_t len = (int64_t)L.len;
        const uint32_t end = (uint32_t)L.len;
        uint64_t base = 0;   // output bytes of the passes before this one
        uint32_t ebase = 0, ocbase = 0, scbase = 0;   // (ALIGN) ... their edits, output code points and source code points
        uint64_t line_edits = 0;
        kgpu_norm_edit *ed = nullptr;
        if constexpr (ALIGN) { line_edits = eoff[i + 1] - eoff[i]; ed = a.edits + eoff[i]; }
        for (int64_t u = 0; u < (int64_t)L.mis + len; u += PASS) {
            const int64_t r0 = u + lane * 16 - (int64_t)L.mis;
            const bool mine = !(r0 + 16 <= 0 || r0 >= len);
            Masks m{0, 0, 0, false};
            uint32_t bytes = 0, n_sc = 0;   // (ALIGN) this lane's source code points ...
            uint64_t n_oc_ed = 0;           // ... and its output code points | edits << 32: ONE counter (two, each added to by one of the two
                                            // lambdas, and the compiler merges the additions into one through a pointer: both counters in scratch)
            if (mine) {
                m = classify(a.t, a.form, L.p, len, r0);
                each_segment(m, len, r0,
                             [&](uint32_t, uint32_t l) {
                                 bytes += l;
                                 if constexpr (ALIGN) ++n_oc_ed;
                             },
                             [&](uint32_t k) {
                                 uint32_t n, next;
                                 const uint32_t r = norm_segment(a.t, a.form, L.p, (uint32_t)(r0 + k), end, buf, n, next);
                                 if (r != NORM_OVERSIZE) {
                                     bytes += r;
                                     if constexpr (ALIGN) n_oc_ed += n | (uint64_t)norm_segment_edit(L.p, (uint32_t)(r0 + k), next, buf, n, r).differs << 32;
                                 }
                             });
                if constexpr (ALIGN) n_sc = (uint32_t)__popc(m.lead & 0xFFFFu);   // the code points that start in this unit
            }
            const uint32_t incl = wave_incl_scan(bytes, lane);   // (a lane has 16 segments of 65 code points at most: 32 bits hold a pass)
            uint64_t o = base + incl - bytes;
            base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            uint32_t e = 0, oc = 0, sc = 0;   // (ALIGN) the line's edits, output and source code points in front of this lane's unit
            if constexpr (ALIGN) {
                const uint32_t n_oc = (uint32_t)n_oc_ed, n_ed = (uint32_t)(n_oc_ed >> 32);
                const uint32_t ie = wave_incl_scan(n_ed, lane), io = wave_incl_scan(n_oc, lane), is = wave_incl_scan(n_sc, lane);
                e = ebase + ie - n_ed; oc = ocbase + io - n_oc; sc = scbase + is - n_sc;
                ebase += (uint32_t)__builtin_amdgcn_readlane((int)ie, 63);
                ocbase += (uint32_t)__builtin_amdgcn_readlane((int)io, 63);
                scbase += (uint32_t)__builtin_amdgcn_readlane((int)is, 63);
            }
            if (!mine) continue;
            // (every store is checked against the line's room: the lengths are the first launch's, and the input may have changed since)
            each_segment(m, len, r0,
                         [&](uint32_t k, uint32_t l) {
                             for (uint32_t j = 0; j < l; ++j, ++o)
                                 if (o < out_len) dst[o] = L.p[r0 + k + j];
                             if constexpr (ALIGN) ++oc;
                         },
                         [&](uint32_t k) {
                             uint32_t n, next;
                             const uint32_t r = norm_segment(a.t, a.form, L.p, (uint32_t)(r0 + k), end, buf, n, next);
                             if (r == NORM_OVERSIZE) return;
                             if constexpr (ALIGN) {   // (every store is checked against the line's scanned edit count, as the text's against its length)
                                 const NormSegEdit d = norm_segment_edit(L.p, (uint32_t)(r0 + k), next, buf, n, r);
                                 if (d.differs) {
                                     if (e < line_edits) {   // kgpu_norm_edit as its six words (the 16-bit pairs put together in registers)
                                         uint32_t *w = (uint32_t *)(ed + e);
                                         w[0] = (uint32_t)o; w[1] = (uint32_t)(r0 + k); w[2] = oc; w[3] = sc + (uint32_t)__popc(m.lead & ((1u << k) - 1u));
                                         w[4] = d.out_len | d.src_len << 16; w[5] = d.out_chars | d.src_chars << 16;
                                     }
                                     ++e;
                                 }
                                 oc += n;
                             }
                             for (uint32_t q = 0; q < n; ++q) {
                                 const uint32_t c = buf.get(q) & 0x1FFFFFu, cl = norm_utf8_len(c);
                                 for (uint32_t j = 0; j < cl; ++j, ++o)
                                     if (o < out_len) dst[o] = norm_utf8_byte(c, j);
                             }
                         });
        }
    }
}

uint32_t normalize_blocks(uint64_t n) { return (uint32_t)(n < 8192 ? (n ? n : 1) : 8192); }

int launch_normalize(const NormArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = normalize_blocks(a.n);
    if (a.n) hipLaunchKernelGGL(k_norm_len<false>, dim3(blocks), dim3(64), 0, st, a);
    RecordsBatch b{};
    b.n = a.n; b.sent_len = a.sent_len; b.text_offsets = a.text_offsets; b.host_ctl = a.host_ctl;
    launch_lines_scan(b, stream);
    if (a.n) hipLaunchKernelGGL(k_norm_write<false>, dim3(blocks), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

int launch_normalize_aligned(const NormAlignArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = normalize_blocks(a.n);
    if (a.n) hipLaunchKernelGGL(k_norm_len<true>, dim3(blocks), dim3(64), 0, st, a);
    RecordsBatch b{}, e{};
    b.n = a.n; b.sent_len = a.sent_len; b.text_offsets = a.text_offsets; b.host_ctl = a.host_ctl;
    launch_lines_scan(b, stream);
    e.n = a.n; e.sent_len = a.edit_len; e.text_offsets = a.edit_offsets; e.host_ctl = a.host_ctl + 1;   // the edits' total: the report's second word
    launch_lines_scan(e, stream);
    if (a.n) hipLaunchKernelGGL(k_norm_write<true>, dim3(blocks), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
