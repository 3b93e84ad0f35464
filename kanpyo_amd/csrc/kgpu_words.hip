// kanpyo_amd/csrc/kgpu_words.hip -- the wakati lines of a batch on the device (include/kanpyo_gpu.h, "wakati-gaki"; not an output of the
// reference): for every sentence ONE line, the words of its kept tokens joined by the separator byte, then '\n'.  A word is the token's
// surface input[position .. position + byte_len) or a name of the handle's pool, as the token's row entry says (kgpu_words_host.cpp builds
// the entries: field, fallback to the surface and the filter are all decided there, per row); the dummy class (EOS) is never a word, and a
// token without a row is a surface that KGPU_WORDS_KEEP drops.
//
// Three launches on the context's stream, the shape of kgpu_format.hip:
//   k_words_len    one wavefront per sentence: sum over its kept tokens of (word bytes + 1), or 1 when nothing is kept -> sent_len[s];
//                  records are range-checked here as line_of checks them
//   k_lines_scan   kgpu_format.hip's, unchanged: exclusive scan, mirrored into the caller's text_offsets, the total published to the host
//   k_words_write  one wavefront per sentence, 64 tokens at a time: the kept ones are compacted (ballot + prefix count) into LDS with their
//                  piece starts (a wave scan), so every piece the lanes search has a byte at least -- the word and one trailing byte, which
//                  is the separator except at the sentence's last byte, which is '\n'; then every lane assembles aligned 16-byte units as
//                  k_lines_write does.  A sentence where nothing is kept gets its lone '\n' from lane 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kgpu_words_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = 4;   // wavefronts per workgroup (one sentence each at a time)

// (one token's word -- Word, word_of -- lives in kgpu_words_dev.h: the word counts share it)

}  // namespace

__global__ __launch_bounds__(256) void k_words_len(WordsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * WPB;
    bool bad = false;
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint64_t k0 = a.tok_offsets[s], k1 = a.tok_offsets[s + 1];
        const uint32_t B = (uint32_t)(a.offsets[s + 1] - a.offsets[s]);
        bad |= k1 < k0;
        uint64_t sum = 0;
        for (uint64_t k = k0 + lane; k < k1; k += 64) {
            const Word w = word_of(a, a.tokens[k], B);
            if (w.kept) sum += (uint64_t)w.len + 1;
            bad |= !w.ok;
        }
        sum = wave_sum64(sum);
        if (lane == 0) {
            a.sent_len[s] = sum ? sum : 1;   // nothing kept: the line is its '\n'
            if (a.status_out) a.status_out[s] = a.status_in[s];
        }
    }
    if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&a.host_ctl[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_words_write(WordsArgs a) {
    __shared__ uint64_t st_s[WPB][64];                                  // piece start, relative to the sentence's first output byte
    __shared__ uint32_t wl_s[WPB][64], src_s[WPB][64], tx_s[WPB][64];   // the word's bytes, where they lie, and in which array
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * WPB + w, nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t *toff = a.sent_len;    // the scan's offsets in device memory
    if (toff[a.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;   // output byte p lives at unit (p + mis) / 16 of `abase`
    uint8_t *const abase = a.text - mis;
    uint64_t *st = st_s[w];
    uint32_t *wl = wl_s[w], *src = src_s[w], *tx = tx_s[w];
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint64_t k0 = a.tok_offsets[s], k1 = a.tok_offsets[s + 1], T0 = toff[s];
        const uint64_t last = toff[s + 1] - T0 - 1;   // the sentence's last byte: its '\n'
        const uint8_t *text = a.utf8 + a.offsets[s];
        const uint32_t B = (uint32_t)(a.offsets[s + 1] - a.offsets[s]);
        uint64_t base = 0;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            const uint32_t m = (uint32_t)(k1 - kw < 64 ? k1 - kw : 64);
            Word wd{0, 0, true, false, true};
            if (lane < m) wd = word_of(a, a.tokens[kw + lane], B);
            const unsigned long long keep = __ballot(wd.kept);
            if (keep == 0) continue;   // (wave-uniform) a window with nothing kept writes nothing
            const uint32_t mk = (uint32_t)__popcll(keep), rank = (uint32_t)__popcll(keep & ((1ull << lane) - 1));
            const uint64_t len = wd.kept ? (uint64_t)wd.len + 1 : 0;
            const uint64_t incl = wave_incl_scan64(len, lane);
            const uint64_t wend = base + lane63(incl);
            wave_sync();   // the previous window's readers are through
            if (wd.kept) { st[rank] = base + incl - len; wl[rank] = wd.len; src[rank] = wd.src; tx[rank] = wd.from_text ? 1u : 0u; }
            wave_sync();
            // this window's bytes: [T0 + base, T0 + wend), in address-aligned 16-byte units
            const uint64_t lo = T0 + base + mis, hi = T0 + wend + mis;
            for (uint64_t u = lo / 16 + lane; u * 16 < hi; u += 64) {
                const uint64_t q0 = u * 16 > lo ? u * 16 : lo, q1 = u * 16 + 16 < hi ? u * 16 + 16 : hi;
                const uint64_t r0 = q0 - mis - T0;   // sentence-relative offset of the unit's first byte of ours
                uint32_t j = 0;                      // the piece holding it: the last j with st[j] <= r0
                for (uint32_t step = 32; step > 0; step >>= 1)
                    if (j + step < mk && st[j + step] <= r0) j += step;
                uint64_t ps = st[j];
                uint32_t cl = wl[j], cp = src[j], ct = tx[j];
                uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
                for (uint32_t b = 0; b < 16; ++b) {
                    const uint64_t q = u * 16 + b;
                    if (q < q0 || q >= q1) continue;
                    const uint64_t r = q - mis - T0;
                    uint64_t rel = r - ps;
                    if (rel > cl) {   // the next piece starts here (every piece has a byte at least)
                        ++j;
                        ps = st[j]; cl = wl[j]; cp = src[j]; ct = tx[j];
                        rel = r - ps;
                    }
                    uint32_t c;
                    if (rel < cl) c = ct ? text[cp + rel] : a.names[cp + rel];
                    else c = r == last ? (uint32_t)'\n' : a.sep;
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
        if (base == 0 && lane == 0) a.text[T0] = '\n';   // no kept token in the whole sentence (a kept one has a byte at least)
    }
}

int launch_format_words(const WordsArgs &a, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((a.n + WPB - 1) / WPB, 8192));
    hipLaunchKernelGGL(k_words_len, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    LinesArgs sc{};   // what k_lines_scan reads and writes
    sc.n = a.n; sc.sent_len = a.sent_len; sc.text_offsets = a.text_offsets; sc.host_ctl = a.host_ctl;
    launch_lines_scan(sc, stream);
    hipLaunchKernelGGL(k_words_write, dim3((unsigned)blocks), dim3(64 * WPB), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
