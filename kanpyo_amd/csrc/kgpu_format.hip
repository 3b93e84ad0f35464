// kanpyo_amd/csrc/kgpu_format.hip -- the `kanpyo tokenize` output of a batch on the device (reference src/bin/kanpyo.rs:174-197):
// for every token one line `surface \t f1,f2,...,fk \n`, where surface is input[position .. position + byte_len] or "EOS" for the dummy
// class, and the features are the dictionary's pre-joined row for the morph (kgpu_features.cpp), empty for the dummy class and for
// id 0 (BOS_EOS_ID, src/lattice/node.rs:3).  A sentence without tokens renders to nothing.
//
// Three launches on the context's stream (kgpu_records_dev.h: launch_render):
//   k_lines_len    sentence_units: a token's line is its surface, '\t', its features, '\n'
//   k_lines_scan   one workgroup, for every render: exclusive scan of sent_len, in place (device memory), mirrored into the caller's text_offsets;
//                  the total published to the host's mapped words
//   k_lines_write  one wavefront per sentence, 64 tokens at a time: their line starts (a wave scan) and fields go to LDS, then write_units.
//                  Nothing is written when the total exceeds the capacity.
#include "kgpu_records_dev.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t EOS_POS = 0xFFFFFFFFu;   // LDS marker: the surface is the literal "EOS"
constexpr uint32_t WPB = RENDER_WPB;

// One token's line: surface (sl bytes at byte `pos` of the sentence, or "EOS"), then '\t', the joined features (fl bytes at feat[fo]), '\n'.
// ok: record_of's.
struct Line { uint32_t sl, pos, fo, fl; bool ok; };
__device__ __forceinline__ Line line_of(const LinesArgs &a, const kgpu_token &t, uint32_t B) {
    if (t.cls == KGPU_CLASS_DUMMY) return Line{3, EOS_POS, 0, 0, true};
    const Record r = record_of(a.b, t, B);
    Line l{0, 0, 0, 0, r.ok};
    if (r.ok) { l.sl = t.byte_len; l.pos = t.position; }
    if (r.has_row) { l.fo = a.feat_off[r.row]; l.fl = a.feat_off[r.row + 1] - l.fo; }   // src/bin/kanpyo.rs:176: BOS_EOS_ID prints no features
    return l;
}

// write_units' pieces: the lines of a window, their fields in the wavefront's LDS rows
struct LinePieces {
    const uint32_t *sl, *pos, *fo, *fl;
    const uint8_t *text, *feat;
    struct Piece { uint32_t sl, pos, fo, fl; };
    __device__ __forceinline__ Piece load(uint32_t j) const { return Piece{sl[j], pos[j], fo[j], fl[j]}; }
    __device__ __forceinline__ uint64_t length(const Piece &p) const { return (uint64_t)p.sl + p.fl + 2; }
    __device__ __forceinline__ uint32_t byte(const Piece &p, uint64_t rel, bool) const {
        if (rel < p.sl) return p.pos == EOS_POS ? (rel == 0 ? 'E' : rel == 1 ? 'O' : 'S') : text[p.pos + rel];
        if (rel == p.sl) return '\t';
        if (rel < (uint64_t)p.sl + 1 + p.fl) return feat[p.fo + (rel - p.sl - 1)];
        return '\n';
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_lines_len(LinesArgs a) {
    sentence_units(a.b, [&](const kgpu_token &t, uint32_t B) { const Line l = line_of(a, t, B); return Units{(uint64_t)l.sl + l.fl + 2, l.ok}; },
                   [](uint64_t sum) { return sum; });
}

// (the pattern of k_scan_counts, kgpu_kernels.hip)
__global__ __launch_bounds__(1024) void k_lines_scan(RecordsBatch a) {
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
    const uint64_t *toff = a.b.sent_len;   // the scan's offsets in device memory (text_offsets may be mapped host memory: a PCIe round trip per read)
    if (toff[a.b.n] > a.text_cap) return;   // the host reports KGPU_ERR_CAPACITY with the size needed
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    uint8_t *const abase = a.text - mis;
    uint64_t *st = st_s[w];
    uint32_t *sl = sl_s[w], *pos = pos_s[w], *fo = fo_s[w], *fl = fl_s[w];
    walk_sentences<WPB, false>(a.b, [&](uint64_t s, uint64_t k0, uint64_t k1, uint32_t B, const uint8_t *text) {
        const uint64_t T0 = toff[s];
        uint64_t base = 0;
        for (uint64_t kw = k0; kw < k1; kw += 64) {
            const uint32_t m = (uint32_t)(k1 - kw < 64 ? k1 - kw : 64);
            Line l{0, 0, 0, 0, true};
            if (lane < m) l = line_of(a, a.b.tokens[kw + lane], B);
            const uint64_t len = lane < m ? (uint64_t)l.sl + l.fl + 2 : 0;
            const uint64_t incl = wave_incl_scan64(len, lane);
            const uint64_t wend = base + lane63(incl);
            wave_sync();   // the previous window's readers are through
            if (lane < m) { st[lane] = base + incl - len; sl[lane] = l.sl; pos[lane] = l.pos; fo[lane] = l.fo; fl[lane] = l.fl; }
            wave_sync();
            write_units(abase, mis, T0, base, wend, 0, st, m, LinePieces{sl, pos, fo, fl, text, a.feat});
            base = wend;
        }
        return false;   // (the length pass has checked the records)
    });
}

void launch_lines_scan(const RecordsBatch &b, void *stream) {
    hipLaunchKernelGGL(k_lines_scan, dim3(1), dim3(b.n > 256 ? 1024 : 256), 0, (hipStream_t)stream, b);
}

int launch_format_lines(const LinesArgs &a, void *stream) { return launch_render(k_lines_len, k_lines_write, a, stream); }

}  // namespace kgpu
