// kanpyo_amd/csrc/kgpu_words.hip -- the wakati lines of a batch on the device (include/kanpyo_gpu.h, "wakati-gaki"; not an output of the
// reference): for every sentence ONE line, the words of its kept tokens joined by the separator byte, then '\n'.  A word is the token's
// surface input[position .. position + byte_len) or a name of the handle's pool, as the token's row entry says (kgpu_words_host.cpp builds
// the entries: field, fallback to the surface and the filter are all decided there, per row); the dummy class (EOS) is never a word, and a
// token without a row is a surface that KGPU_WORDS_KEEP drops.
//
// Three launches on the context's stream (kgpu_records_dev.h: launch_render):
//   k_words_len    sentence_units: a kept token gives its word's bytes + 1; a sentence where nothing is kept is its '\n'
//   k_lines_scan   kgpu_format.hip's
//   k_words_write  one wavefront per sentence, 64 tokens at a time: the kept ones are compacted (ballot + prefix count) into LDS with their
//                  piece starts (a wave scan), so every piece the lanes search has a byte at least -- the word and one trailing byte, which
//                  is the separator except at the sentence's last byte, which is '\n'; then write_units.  A sentence where nothing is kept
//                  gets its lone '\n' from lane 0.
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t WPB = RENDER_WPB;

// write_units' pieces: the kept words of a window and their trailing byte, their fields in the wavefront's LDS rows
struct WordPieces {
    const uint32_t *wl, *src, *tx;   // the word's bytes, where they lie, and in which array
    const uint8_t *text, *names;
    uint32_t sep;
    struct Piece { uint32_t len, src, tx; };
    __device__ __forceinline__ Piece load(uint32_t j) const { return Piece{wl[j], src[j], tx[j]}; }
    __device__ __forceinline__ uint64_t length(const Piece &p) const { return (uint64_t)p.len + 1; }
    __device__ __forceinline__ uint32_t byte(const Piece &p, uint64_t rel, bool last) const {
        if (rel < p.len) return p.tx ? text[p.src + rel] : names[p.src + rel];
        return last ? (uint32_t)'\n' : sep;
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_words_len(WordsArgs a) {
    sentence_units(a.b, [&](const kgpu_token &t, uint32_t B) { const Word w = word_of(a.b, a.w, t, B); return Units{w.kept ? (uint64_t)w.len + 1 : 0, w.ok}; },
                   [](uint64_t sum) { return sum ? sum : 1; });   // nothing kept: the line is its '\n'
}

__global__ __launch_bounds__(256) void k_words_write(WordsArgs a) {
    __shared__ uint64_t st_s[WPB][64];                                  // piece start, relative to the sentence's first output byte
    __shared__ uint32_t wl_s[WPB][64], src_s[WPB][64], tx_s[WPB][64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t *toff = a.b.sent_len;    // the scan's offsets in device memory
    if (toff[a.b.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    uint8_t *const abase = a.text - mis;
    uint64_t *st = st_s[w];
    uint32_t *wl = wl_s[w], *src = src_s[w], *tx = tx_s[w];
    walk_sentences<WPB, false>(a.b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        const uint64_t T0 = toff[s];
        const uint64_t last = toff[s + 1] - T0 - 1;   // the sentence's last byte: its '\n'
        uint64_t base = 0;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            const uint32_t m = (uint32_t)(k1 - kw < 64 ? k1 - kw : 64);
            Word wd{0, 0, true, false, true};
            if (lane < m) wd = word_of(a.b, a.w, a.b.tokens[kw + lane], B);
            const unsigned long long keep = __ballot(wd.kept);
            if (keep == 0) continue;   // (wave-uniform) a window with nothing kept writes nothing
            const uint32_t mk = (uint32_t)__popcll(keep), rank = (uint32_t)__popcll(keep & ((1ull << lane) - 1));
            const uint64_t len = wd.kept ? (uint64_t)wd.len + 1 : 0;
            const uint64_t incl = wave_incl_scan64(len, lane);
            const uint64_t wend = base + lane63(incl);
            wave_sync();   // the previous window's readers are through
            if (wd.kept) { st[rank] = base + incl - len; wl[rank] = wd.len; src[rank] = wd.src; tx[rank] = wd.from_text ? 1u : 0u; }
            wave_sync();
            write_units(abase, mis, T0, base, wend, last, st, mk, WordPieces{wl, src, tx, text, a.w.names, a.w.sep});
            base = wend;
        }
        if (base == 0 && lane == 0) a.text[T0] = '\n';   // no kept token in the whole sentence (a kept one has a byte at least)
        return false;   // (the length pass has checked the records)
    });
}

int launch_format_words(const WordsArgs &a, void *stream) { return launch_render(k_words_len, k_words_write, a, stream); }

}  // namespace kgpu
