// kanpyo_amd/csrc/kgpu_format.hip -- the `kanpyo tokenize` output of a batch on the device (reference src/bin/kanpyo.rs:174-197):
// for every token one line `surface \t f1,f2,...,fk \n`, where surface is input[position .. position + byte_len] or "EOS" for the dummy
// class, and the features are the dictionary's pre-joined row for the morph (kgpu_features.cpp), empty for the dummy class and for
// id 0 (BOS_EOS_ID, src/lattice/node.rs:3).  A sentence without tokens renders to nothing.
//
// Three launches on the context's stream:
//   k_lines_len    one wavefront per sentence: its tokens' line lengths summed -> sent_len[s]; records are range-checked here
//   k_lines_scan   one workgroup: exclusive scan of sent_len, in place (device memory), mirrored into the caller's text_offsets;
//                  the total published to the host's mapped words
//   k_lines_write  one wavefront per sentence, 64 tokens at a time: their line starts (a wave scan) go to LDS, then every lane
//                  assembles one aligned 16-byte unit of the output from the surface, '\t', the feature bytes and '\n' and stores
//                  it whole; only the units a window of tokens shares with its neighbours (a sentence's head and tail, and the
//                  ends of the caller's buffer) are stored byte by byte.  Nothing is written when the total exceeds the capacity.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_device.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t EOS_POS = 0xFFFFFFFFu;   // LDS marker: the surface is the literal "EOS"
constexpr uint32_t WPB = 4;                 // wavefronts per workgroup (one sentence each at a time)

// One token's line: surface (sl bytes at byte `pos` of the sentence, or "EOS"), then '\t', the joined features (fl bytes at feat[fo]), '\n'.
// ok = false: the record is not one the tokenizer could have written for this sentence and dictionary (class, id or surface out of range).
struct Line { uint32_t sl, pos, fo, fl; bool ok; };
__device__ __forceinline__ Line line_of(const LinesArgs &a, const kgpu_token &t, uint32_t B) {
    Line l{0, 0, 0, 0, true};
    if (t.cls == KGPU_CLASS_DUMMY) { l.sl = 3; l.pos = EOS_POS; return l; }
    l.sl = t.byte_len; l.pos = t.position;
    l.ok = t.cls <= KGPU_CLASS_UNKNOWN && t.position <= B && t.byte_len <= B - t.position;
    if (t.id != 0) {   // src/bin/kanpyo.rs:176: BOS_EOS_ID prints no features
        const uint32_t id = (uint32_t)t.id, lim = t.cls == KGPU_CLASS_KNOWN ? a.n_morph : a.n_rows - a.n_morph;
        if (l.ok && t.id > 0 && id <= lim) {
            const uint32_t row = (t.cls == KGPU_CLASS_KNOWN ? 0u : a.n_morph) + id - 1;
            l.fo = a.feat_off[row]; l.fl = a.feat_off[row + 1] - l.fo;
        } else {
            l.ok = false;
        }
    }
    if (!l.ok) l = Line{0, 0, 0, 0, false};
    return l;
}

}  // namespace

__global__ __launch_bounds__(256) void k_lines_len(LinesArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    bool bad = false;
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint64_t k0 = a.tok_offsets[s], k1 = a.tok_offsets[s + 1];
        const uint32_t B = (uint32_t)(a.offsets[s + 1] - a.offsets[s]);
        bad |= k1 < k0;
        uint64_t sum = 0;
        for (uint64_t k = k0 + lane; k < k1; k += 64) {
            const Line l = line_of(a, a.tokens[k], B);
            sum += (uint64_t)l.sl + l.fl + 2;
            bad |= !l.ok;
        }
        sum = wave_sum64(sum);
        if (lane == 0) {
            a.sent_len[s] = sum;
            if (a.status_out) a.status_out[s] = a.status_in[s];
        }
    }
    if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&a.host_ctl[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (the pattern of k_scan_counts, kgpu_kernels.hip)
__global__ __launch_bounds__(1024) void k_lines_scan(LinesArgs a) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < a.n; base += nthr) {
        const uint64_t i = base + tid;
        const uint64_t v = i < a.n ? a.sent_len[i] : 0;
        const uint64_t vs = wave_incl_scan64(v, lane);
        if (lane == 63) wsum[wid] = vs;
        __syncthreads();
        uint64_t woff = 0;
        for (uint32_t w = 0; w < wid; ++w) woff += wsum[w];
        const uint64_t carry = carry_s;
        if (i < a.n) a.sent_len[i] = a.text_offsets[i] = carry + woff + vs - v;   // (each thread reads its element before it writes it)
        __syncthreads();
        if (tid == nthr - 1) carry_s = carry + woff + vs;
        __syncthreads();
    }
    if (tid == 0) {
        a.sent_len[a.n] = a.text_offsets[a.n] = carry_s;
        __hip_atomic_store(&a.host_ctl[0], (unsigned long long)carry_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(256) void k_lines_write(LinesArgs a) {
    __shared__ uint64_t st_s[WPB][64];                                  // line start, relative to the sentence's first output byte
    __shared__ uint32_t sl_s[WPB][64], pos_s[WPB][64], fo_s[WPB][64], fl_s[WPB][64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + w, nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t *toff = a.sent_len;   // the scan's offsets in device memory (text_offsets may be mapped host memory: a PCIe round trip per read)
    if (toff[a.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    // 16-byte units are aligned in the address space: output byte p lives at unit (p + mis) / 16 of `abase`
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    uint8_t *const abase = a.text - mis;
    uint64_t *st = st_s[w];
    uint32_t *sl = sl_s[w], *pos = pos_s[w], *fo = fo_s[w], *fl = fl_s[w];
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint64_t k0 = a.tok_offsets[s], k1 = a.tok_offsets[s + 1], T0 = toff[s];
        const uint8_t *text = a.utf8 + a.offsets[s];
        const uint32_t B = (uint32_t)(a.offsets[s + 1] - a.offsets[s]);
        uint64_t base = 0;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            const uint32_t m = (uint32_t)(k1 - kw < 64 ? k1 - kw : 64);
            Line l{0, 0, 0, 0, true};
            if (lane < m) l = line_of(a, a.tokens[kw + lane], B);
            const uint64_t len = lane < m ? (uint64_t)l.sl + l.fl + 2 : 0;
            const uint64_t incl = wave_incl_scan64(len, lane);
            const uint64_t wend = base + lane63(incl);
            wave_sync();   // the previous window's readers are through
            if (lane < m) { st[lane] = base + incl - len; sl[lane] = l.sl; pos[lane] = l.pos; fo[lane] = l.fo; fl[lane] = l.fl; }
            wave_sync();
            // this window's bytes: [T0 + base, T0 + wend), in address-aligned 16-byte units
            const uint64_t lo = T0 + base + mis, hi = T0 + wend + mis;
            for (uint64_t u = lo / 16 + lane; u * 16 < hi; u += 64) {
                const uint64_t q0 = u * 16 > lo ? u * 16 : lo, q1 = u * 16 + 16 < hi ? u * 16 + 16 : hi;
                const uint64_t r0 = q0 - mis - T0;   // sentence-relative offset of the unit's first byte of ours
                uint32_t j = 0;                      // the line holding it: the last j with st[j] <= r0
                for (uint32_t step = 32; step > 0; step >>= 1)
                    if (j + step < m && st[j + step] <= r0) j += step;
                uint64_t ls = st[j];
                uint32_t cs = sl[j], cp = pos[j], cfo = fo[j], cfl = fl[j];
                uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
                for (uint32_t b = 0; b < 16; ++b) {
                    const uint64_t q = u * 16 + b;
                    if (q < q0 || q >= q1) continue;
                    uint64_t rel = q - mis - T0 - ls;
                    if (rel >= (uint64_t)cs + cfl + 2) {   // the next line starts here (every line has 2 bytes or more)
                        ++j;
                        ls = st[j]; cs = sl[j]; cp = pos[j]; cfo = fo[j]; cfl = fl[j];
                        rel = q - mis - T0 - ls;
                    }
                    uint32_t c;
                    if (rel < cs) c = cp == EOS_POS ? (rel == 0 ? 'E' : rel == 1 ? 'O' : 'S') : text[cp + rel];
                    else if (rel == cs) c = '\t';
                    else if (rel < (uint64_t)cs + 1 + cfl) c = a.feat[cfo + (rel - cs - 1)];
                    else c = '\n';
                    word[b >> 2] |= c << (8 * (b & 3));
                }
                if (q0 == u * 16 && q1 == u * 16 + 16) {
                    *(uint4 *)(abase + u * 16) = make_uint4(word[0], word[1], word[2], word[3]);
                } else {   // a unit shared with the neighbouring window, sentence or the bytes outside the buffer: ours only
                    for (uint64_t q = q0; q < q1; ++q) abase[q] = (uint8_t)(word[(q & 15) >> 2] >> (8 * (q & 3)));
                }
            }
            base = wend;
        }
    }
}

void launch_lines_scan(const LinesArgs &a, void *stream) {
    hipLaunchKernelGGL(k_lines_scan, dim3(1), dim3(a.n > 256 ? 1024 : 256), 0, (hipStream_t)stream, a);
}

int launch_format_lines(const LinesArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.n + WPB - 1) / WPB, 8192));
    hipLaunchKernelGGL(k_lines_len, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    launch_lines_scan(a, stream);
    hipLaunchKernelGGL(k_lines_write, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
