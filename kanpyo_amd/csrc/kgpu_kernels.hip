// kanpyo_amd/csrc/kgpu_kernels.hip -- hand-written gfx950 (CDNA4) kernels for
// the Tokenizer::tokenize hot path (reference src/tokenizer.rs:16-45).
//
// One 64-lane wavefront owns one sentence from UTF-8 bytes to token records:
//   phase 0  UTF-8 decode + validation, char -> byte offset, char category
//            (char_category_def.rs:33-38)
//   phase 1  lattice COUNT: one lane per start position walks the double array
//            (trie/da.rs:155-182), expands duplicates (index.rs:46-51), decides the
//            unknown-word span (lattice.rs:42-99); per-position node counts and
//            per-end-position bucket counts
//   phase 2  wave prefix sums -> node numbering in reference insertion order
//            (lattice.rs:105-110) and bucket offsets (= Lattice.edges, lattice.rs:9)
//   phase 3  lattice EMIT: same walk, nodes written to their numbered slots
//   phase 4  Viterbi sweep over start positions (lattice.rs:116-142): all nodes
//            starting at q share the predecessor bucket edges[q]; lanes take
//            targets, the bucket is broadcast; min is lexicographic on
//            (total, predecessor index) = strict '<' over ascending insertion order
//   phase 5  backtrace (lattice.rs:144-153) + Node -> Token (tokenizer.rs:22-43)
// Integer/indexing work only: no MFMA anywhere.
//
// This file holds the GENERAL kernel: every per-sentence array lives in a bump-allocated HBM scratch slab and every
// step of the Viterbi chain is a global-memory round trip -- no LDS at all, so its workgroups start on a CU whose LDS is
// fully taken, and any sentence length / lattice shape works.  It is the LAST RESORT of the launch chain (what the LDS-resident
// pool kernel, kgpu_pool.hip, and the windowed kernel, kgpu_window.hip, cannot hold) and the kernel behind kgpu_lattice_dump: its
// slabs ARE the lattice.  (Round 2-3 also instantiated it with an LDS-blocked sweep as "the long-sentence kernel"; the windowed kernel
// took that place in round 4.)  Also here: the scan / compaction kernels, and the thin launchers of a chain's steps (the chain itself: kgpu_chain.cpp).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kgpu_chain.h"
#include "kgpu_device.h"

namespace kgpu {

using namespace dev;

namespace {

constexpr uint32_t GMAXM = 8;  // trie matches parked per start position by the count walk

}  // namespace

__global__ __launch_bounds__(64) void k_tokenize_general(DictView d, BatchArgs a, WorkIO io, uint32_t stop_after /* ablation timing only */) {
    const uint32_t lane = threadIdx.x;
    Slab sa{nullptr, 0}, sn{nullptr, 0};
    const int32_t base_root = d.da[1].base;
    uint64_t accW[7] = {0, 0, 0, 0, 0, 0, 0};  // work counters of this workgroup, flushed once at exit

    for (uint32_t iter = 0;; ++iter) {
        uint64_t s = 0;
        if (!work_next(io, a, iter, s)) break;

        const uint64_t b0 = a.offsets[s];
        const uint32_t B = (uint32_t)(a.offsets[s + 1] - b0);
        const uint8_t *text = a.utf8 + b0;

        // ---- slab A: per-char arrays (C <= B) --------------------------------
        const uint64_t na = (uint64_t)B + 4;
        // (keep_lattice: the sentence's own slabs, left behind for the graphviz passes; the descriptor table is zero where a sentence leaves early)
        unsigned long long *const eos_dp = a.keep_lattice ? a.lat_desc + LAT_DESC_WORDS * s + LAT_EOS_DP : a.dump_lattice ? &a.ctl->dump[LAT_EOS_DP] : nullptr;
        if (!(a.keep_lattice ? slab_fresh(sa, na * (28 + 5 * GMAXM) + 64, a, lane) : slab_ensure(sa, na * (28 + 5 * GMAXM) + 64, a, lane))) {
            if (lane == 0) { a.status[s] = KGPU_SENT_NO_SCRATCH; a.tok_count[s] = 0; }
            continue;
        }
        uint32_t *cbyte = (uint32_t *)sa.ptr;  // char -> byte offset, [C] = B
        uint32_t *uspan = cbyte + na;          // unknown span in chars (0 = none)
        uint32_t *nb = uspan + na;             // node count, then first node index, per start
        uint32_t *boff = nb + na;              // bucket count, then offset, per end
        uint32_t *bfill = boff + na;           // bucket fill cursor
        uint32_t *path = bfill + na;           // backtrace
        uint32_t *mid = path + na;             // [na][GMAXM] trie ids parked by the count walk (the emit phase re-walks nothing)
        uint16_t *cp16 = (uint16_t *)(mid + na * GMAXM);  // BMP code point (0xFFFF: not BMP)
        uint8_t *ccat = (uint8_t *)(cp16 + na);
        uint8_t *mcnt = ccat + na;             // parked matches per start position (0xFF: more than GMAXM -> re-walk)
        uint8_t *mnch = mcnt + na;             // [na][GMAXM] match length in chars

        // ---- phase 0: decode ------------------------------------------------
        const bool ct = d.da2 != nullptr;  // character-level trie (kgpu_chartrie.cpp): the walks read character codes, not bytes; cp16[] then holds the codes
        uint32_t C = 0, bad = 0, lensum = 0;
        for (uint32_t k0 = 0; k0 < B; k0 += 64) {
            uint32_t k = k0 + lane;
            uint32_t b = k < B ? text[k] : 0x80u;
            bool start = k < B && (b & 0xC0) != 0x80;
            uint64_t m = __ballot(start);
            uint32_t ci = C + __popcll(m & ((1ull << lane) - 1));
            if (start) {
                uint32_t cp;
                const uint32_t l = utf8_decode_lead(b, k, B, [&](uint32_t kk) -> uint32_t { return text[kk]; }, cp, bad);
                lensum += l;
                cbyte[ci] = k;
                uint32_t code = cp < 0xFFFFu ? cp : 0xFFFFu;
                if (ct) code = cp < 0xFFFFu ? (uint32_t)d.crec[cp].code : (d.n_nb ? ct_code_nonbmp(d, cp) : 0xFFFFu);
                cp16[ci] = (uint16_t)code;
                // char_category_def.rs:33-38: table[ch] if in range else table[0]
                ccat[ci] = bad ? 0 : (cp < d.cat_len ? d.cat[cp] : d.cat[0]);
            }
            C += __popcll(m);
        }
        lensum = bcast32(wave_sum(lensum));  // keep every early exit wave-uniform (SGPR) for the compiler
        if (__ballot(bad != 0) != 0 || lensum != B) {  // stray continuation bytes leave lensum < B
            if (lane == 0) { a.status[s] = KGPU_SENT_INVALID_UTF8; a.tok_count[s] = 0; }
            continue;
        }
        if (lane == 0) { cbyte[C] = B; if (ct) cp16[C] = 0xFFFFu; }
        uint32_t *cnt_e = boff, *fill_e = bfill;  // per-end-position counters / fill cursors (global atomics)
        const uint8_t *wtext = text;
        auto code_at = [&](uint32_t j) -> uint32_t { return (uint32_t)cp16[min(j, C)]; };  // ([C]: none)
        for (uint32_t e = lane; e < C + 3; e += 64) { cnt_e[e] = 0; bfill[e] = 0; }
        __syncthreads();

        // ---- phase 1: count ----------------------------------------------------
        const int nchunks = (int)((C + 63) / 64);
        uint32_t carry_end = C;
        uint32_t wT = 0, wE = 0;  // work counters (only reduced when a.count_work)
        // two chunks of 64 start positions per round, walked side by side (da_walk_first2): a chunk costs its longest
        // walk, a pair the longer of the two -- not their sum (the count walk is 21-28 % of this kernel)
        for (int ch = nchunks - 1; ch >= 0; ch -= 2) {
            uint32_t iX[2], catX[2], runX[2], cntX[2] = {0, 0}, mX[2] = {0, 0};
            bool actX[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {  // x = 0: chunk ch, x = 1: chunk ch - 1 (run ends carry from the later chunk to the earlier)
                const bool have = ch - x >= 0;
                const uint32_t i = have ? (uint32_t)(ch - x) * 64 + lane : 0xFFFFFFF0u;
                const bool active = have && i < C;
                const uint32_t cat = active ? ccat[i] : 0x1FFu;
                const uint32_t ncat = (have && i + 1 < C) ? ccat[i + 1] : 0x2FFu;
                const uint64_t bm = __ballot(active && ncat != cat);
                const uint64_t rest = bm >> lane;
                const uint32_t run_end = rest ? i + (uint32_t)__ffsll((unsigned long long)rest) : carry_end;
                if (have) carry_end = bcast32(run_end);
                iX[x] = i; actX[x] = active; catX[x] = cat; runX[x] = run_end;
            }
            auto on_match = [&](int x) {
                return [&, x](uint32_t id, uint32_t nch, uint32_t dup) {
                    const uint32_t i = iX[x];
                    uint32_t &m = mX[x];
                    if (m < GMAXM && nch < 256) { mid[(size_t)i * GMAXM + m] = id; mnch[(size_t)i * GMAXM + m] = (uint8_t)nch; }
                    else m = 0x100;  // does not fit the parking area: the emit phase walks again
                    ++m;
                    uint32_t nrec = 1u + (dup != NONE ? dup : (uint32_t)d.morph[id - 1].dup);  // index.rs:46-51
                    cntX[x] += nrec;
                    atomicAdd(&cnt_e[i + nch], nrec);
                };
            };
            uint32_t cpX[2], kbX[2], knX[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) { cpX[x] = actX[x] ? cp16[iX[x]] : 0xFFFFu; kbX[x] = actX[x] ? cbyte[iX[x]] : 0u; knX[x] = actX[x] ? cbyte[iX[x] + 1] : 0u; }
            if (ct) {
                ct_walk2(d, actX[0], [&](uint32_t dep) { return code_at(iX[0] + dep); }, on_match(0), actX[1], [&](uint32_t dep) { return code_at(iX[1] + dep); }, on_match(1));
                if (a.count_work == 1u) {  // the reference's byte steps (work counters; not with KGPU_PROFILE_NO_T)
#pragma unroll
                    for (int x = 0; x < 2; ++x) if (actX[x]) wT += da_walk(d, text, kbX[x], B, base_root, [](uint32_t, uint32_t, uint32_t) {});
                }
            } else
            wT += da_walk_first2(d, wtext, B, actX[0] && cpX[0] != 0xFFFFu, cpX[0], kbX[0], knX[0], on_match(0),
                                 actX[1] && cpX[1] != 0xFFFFu, cpX[1], kbX[1], knX[1], on_match(1));
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                if (!actX[x]) continue;
                const uint32_t i = iX[x];
                if (!ct && cpX[x] == 0xFFFFu) wT += da_walk(d, wtext, kbX[x], B, base_root, on_match(x));  // first character outside the BMP: no table entry
                uint32_t cnt = cntX[x];
                const uint32_t m = mX[x];
                mcnt[i] = (uint8_t)(m > GMAXM ? 0xFFu : m);
                const CatInfo ci = d.cinfo[catX[x]];
                uint32_t span = 0;
                // lattice.rs:54: !matched_known || invoke_list[cat]; lattice.rs:87-92: no unk entry -> nothing
                if ((cnt == 0 || (ci.flags & CAT_INVOKE)) && (ci.flags & CAT_HAS_UNK) && ci.unk_count) {
                    span = 1;
                    if (ci.flags & CAT_GROUP) {  // lattice.rs:66-84
                        uint32_t r = runX[x] - i;
                        span = r < MAX_UNKNOWN_LEN ? r : MAX_UNKNOWN_LEN;
                    }
                    cnt += ci.unk_count;
                    atomicAdd(&cnt_e[i + span], ci.unk_count);
                }
                uspan[i] = span;
                nb[i] = cnt;
            }
        }
        if (lane == 0) {
            nb[C] = 1;      // EOS starts at C (lattice.rs:165-175)
            nb[C + 1] = 0;
            atomicAdd(&cnt_e[0], 1u);  // BOS ends at 0 (lattice.rs:156-164)
        }
        __syncthreads();

#define KGPU_GSTOP(k) if (stop_after == (k)) { if (lane == 0) { a.status[s] = KGPU_SENT_TRUNCATED; a.tok_count[s] = 0; } continue; }
        KGPU_GSTOP(3)
        // ---- phase 2: prefix sums ------------------------------------------------
        uint32_t ncarry = 1, bcarry = 0;  // node 0 is BOS
        for (uint32_t i0 = 0; i0 < C + 2; i0 += 64) {
            const uint32_t i = i0 + lane;
            const uint32_t v = i < C + 2 ? nb[i] : 0;
            const uint32_t w = i < C + 2 ? ld_l2(&boff[i]) : 0;  // updated by L2 atomics
            const uint32_t vs = wave_incl_scan(v, lane), ws = wave_incl_scan(w, lane);
            if (i < C + 2) { nb[i] = ncarry + vs - v; boff[i] = bcarry + ws - w; }
            ncarry += __shfl(vs, 63, 64);
            bcarry += __shfl(ws, 63, 64);
        }
        const uint32_t N = bcast32(ncarry);  // BOS + words + EOS (scalarised: the slab test must be wave-uniform)
        __syncthreads();

        // ---- slab N: per-node arrays -----------------------------------------------
        if (!(a.keep_lattice ? slab_fresh(sn, lat_scratch_off(N) + lat_scratch_bytes(N) + 64, a, lane) : slab_ensure(sn, (uint64_t)N * 44 + 64, a, lane))) {
            if (lane == 0) { a.status[s] = KGPU_SENT_NO_SCRATCH; a.tok_count[s] = 0; }
            continue;
        }
        uint4 *nodeA = (uint4 *)sn.ptr;   // {left | right << 16, cost, bucket slot, signed id}
        uint4 *bucket = nodeA + N;        // {dp, right_id, node index, -}
        uint2 *nodeB = (uint2 *)(bucket + N);  // {start char, end char}
        uint32_t *pre = (uint32_t *)(nodeB + N);

        // ---- phase 3: emit -----------------------------------------------------------
        for (uint32_t i = lane; i < C; i += 64) {
            uint32_t t = nb[i];
            auto emit_match = [&](uint32_t id, uint32_t nch, uint32_t /*dup*/ = 0) {
                const uint32_t end = i + nch;
                const Morph8 m0 = d.morph[id - 1];  // first record: carries the duplicate count (index.rs:46-51)
                const uint32_t nrec = 1u + m0.dup;
                for (uint32_t r = 0; r < nrec; ++r) {  // lattice.rs:177-188
                    const Morph8 m = r ? d.morph[id - 1 + r] : m0;
                    const uint32_t slot = boff[end] + atomicAdd(&fill_e[end], 1u);
                    nodeA[t] = make_uint4((uint16_t)m.left | ((uint32_t)(uint16_t)m.right << 16),
                                          (uint32_t)(int32_t)m.cost, slot, id + r);
                    nodeB[t] = make_uint2(i, end);
                    bucket[slot] = make_uint4((uint32_t)INF, (uint16_t)m.right, t, 0);  // dp is filled in by the sweep
                    ++t;
                }
            };
            const uint32_t nm = mcnt[i];
            if (nm == 0xFFu) {
                if (ct) ct_walk(d, 1, d.da2[1].base, 0, [&](uint32_t dep) { return code_at(i + dep); }, emit_match, 0u);
                else da_walk(d, wtext, cbyte[i], B, base_root, emit_match);
            }
            else for (uint32_t m = 0; m < nm; ++m) emit_match(mid[(size_t)i * GMAXM + m], mnch[(size_t)i * GMAXM + m]);
            const uint32_t span = uspan[i];
            if (span) {  // lattice.rs:87-97,190-201
                const CatInfo ci = d.cinfo[ccat[i]];
                const uint32_t end = i + span;
                for (uint32_t r = 0; r < ci.unk_count; ++r) {
                    const Morph8 m = d.unk_morph[ci.unk_first - 1 + (int32_t)r];
                    const uint32_t slot = boff[end] + atomicAdd(&fill_e[end], 1u);
                    nodeA[t] = make_uint4((uint16_t)m.left | ((uint32_t)(uint16_t)m.right << 16),
                                          (uint32_t)(int32_t)m.cost, slot,
                                          (uint32_t)(-(ci.unk_first + (int32_t)r)));
                    nodeB[t] = make_uint2(i, end);
                    bucket[slot] = make_uint4((uint32_t)INF, (uint16_t)m.right, t, 0);
                    ++t;
                }
            }
        }
        if (lane == 0) {
            nodeA[N - 1] = make_uint4(d.eos_left, 0, NONE, 0);  // EOS: Morph(0,0,0), id 0 (context id 0 in its ranked numbering)
            nodeB[N - 1] = make_uint2(C, C);
            bucket[0] = make_uint4(0, d.bos_right, 0, 0);  // BOS: dp None -> 0 (lattice.rs:127)
            pre[0] = NONE;
            if (a.keep_lattice) { nodeA[0] = make_uint4(d.bos_right << 16, 0, 0, 0); nodeB[0] = make_uint2(0, 0); }  // BOS as a node like the others (the dump does not read these)
        }
        __syncthreads();

        KGPU_GSTOP(5)
        // ---- phase 4: Viterbi sweep ---------------------------------------------------
        // one position through global memory (lattice.rs:116-142): lanes take targets, every lane
        // walks the whole predecessor bucket
        auto global_step = [&](uint32_t q) {
            const uint32_t t0 = nb[q], t1 = nb[q + 1], p0 = boff[q], P = boff[q + 1] - p0;
            wE += (lane == 0) ? P * (t1 - t0) : 0;
            if (P >= 48) {
                // wide bucket (e.g. every unknown word of a 1024-char run ends at the same position): the lanes
                // share one target at a time and split its predecessors -- coalesced bucket reads, P/64 steps
                for (uint32_t t = t0; t < t1; ++t) {
                    const uint4 na_ = nodeA[t];
                    const int16_t *col = d.conn + (size_t)d.conn_rows * (na_.x & 0xFFFFu);
                    int32_t best = 0x7FFFFFFF;
                    uint32_t bidx = NONE;
                    for (uint32_t j = lane; j < P; j += 64) {
                        const uint4 e = bucket[p0 + j];
                        const int32_t v = (int32_t)e.x + (int32_t)col[e.y];
                        if (v < best || (v == best && e.z < bidx)) { best = v; bidx = e.z; }
                    }
                    const int32_t vmin = wave_min_i32(best);
                    const uint32_t nmin = wave_min_u32(best == vmin ? bidx : NONE);
                    if (lane == 0) {
                        const int32_t tot = vmin + (int32_t)na_.y;  // min(.., INF) then strict '<' INF
                        const bool ok = tot < INF;
                        pre[t] = ok ? nmin : NONE;
                        if (na_.z != NONE) bucket[na_.z].x = (uint32_t)(ok ? tot : INF);
                        else if (eos_dp) *eos_dp = (unsigned long long)(uint32_t)(ok ? tot : INF);  // EOS has no bucket entry
                    }
                }
                __syncthreads();
                return;
            }
            for (uint32_t t = t0 + lane; t < t1; t += 64) {
                const uint4 na_ = nodeA[t];
                const int16_t *col = d.conn + (size_t)d.conn_rows * (na_.x & 0xFFFFu);
                int32_t best = 0x7FFFFFFF;
                uint32_t bidx = NONE;
                for (uint32_t j = 0; j < P; ++j) {
                    const uint4 e = bucket[p0 + j];
                    const int32_t v = (int32_t)e.x + (int32_t)col[e.y];
                    if (v < best || (v == best && e.z < bidx)) { best = v; bidx = e.z; }
                }
                int32_t dpv = INF;
                uint32_t prv = NONE;
                if (P) {
                    const int32_t tot = best + (int32_t)na_.y;  // min(.., INF) then strict '<' INF
                    if (tot < INF) { dpv = tot; prv = bidx; }
                }
                pre[t] = prv;
                if (na_.z != NONE) bucket[na_.z].x = (uint32_t)dpv;
                else if (eos_dp) *eos_dp = (unsigned long long)(uint32_t)dpv;  // EOS has no bucket entry
            }
            __syncthreads();
        };
        for (uint32_t q = 0; q <= C; ++q) global_step(q);
        wE = wave_sum(wE);

        KGPU_GSTOP(7)
        // ---- phase 5: backtrace + tokens -----------------------------------------------
        uint32_t K = 0;
        if (lane == 0) {
            uint32_t pos = N - 1, pr;
            while ((pr = pre[pos]) != NONE && K <= C) { path[K++] = pos; pos = pr; }  // K <= C + 1 always; bound the walk anyway
        }
        K = bcast32(K);
        // staging slot of the sentence: K <= C + 1 <= B + 1 tokens always fit at b0 + s
        // (no cursor atomics: a single hot word serialises ~90 sentences/us chip-wide)
        const uint64_t ts = b0 - a.offsets[0] + s;
        __syncthreads();
        {
            for (uint32_t k = lane; k < K; k += 64) {
                const uint32_t t = path[K - 1 - k];
                const int32_t sid = (int32_t)nodeA[t].w;
                const uint2 se = nodeB[t];
                kgpu_token tk;
                if (sid == 0) {  // Dummy -> "EOS" (tokenizer.rs:27-28,34)
                    tk.id = 0; tk.cls = KGPU_CLASS_DUMMY; tk.position = B; tk.start = C; tk.end = C + 3; tk.byte_len = 0;
                } else {
                    const uint32_t bs = cbyte[se.x];
                    tk.id = sid > 0 ? sid : -sid;
                    tk.cls = sid > 0 ? KGPU_CLASS_KNOWN : KGPU_CLASS_UNKNOWN;
                    tk.position = bs; tk.start = se.x; tk.end = se.y; tk.byte_len = cbyte[se.y] - bs;
                }
                a.stage[ts + k] = tk;
            }
        }
        if (lane == 0) { a.status[s] = KGPU_SENT_OK; a.tok_count[s] = K; }
        if (a.dump_lattice && lane == 0) {  // kgpu_lattice_dump: the host reads the lattice straight out of the two slabs
            a.ctl->dump[LAT_SLAB_A] = (unsigned long long)(sa.ptr - a.arena); a.ctl->dump[LAT_SLAB_N] = (unsigned long long)(sn.ptr - a.arena);
            a.ctl->dump[LAT_B] = B; a.ctl->dump[LAT_C] = C; a.ctl->dump[LAT_N] = N; a.ctl->dump[LAT_VALID] = 1;
        }
        if (a.keep_lattice && lane == 0) {
            unsigned long long *ds = a.lat_desc + LAT_DESC_WORDS * s;
            ds[LAT_SLAB_A] = (unsigned long long)(sa.ptr - a.arena); ds[LAT_SLAB_N] = (unsigned long long)(sn.ptr - a.arena);
            ds[LAT_B] = B; ds[LAT_C] = C; ds[LAT_N] = N; ds[LAT_VALID] = 1;
        }
        if (a.count_work) {
            wT = wave_sum(wT);
            accW[0] += 1; accW[1] += B; accW[2] += C; accW[3] += wT; accW[4] += N - 1; accW[5] += bcast32(wE); accW[6] += K;
        }
        __syncthreads();
    }
    if (a.count_work && lane == 0)
        for (int k = 0; k < 7; ++k) atomicAdd(&a.ctl->work[k], (unsigned long long)accW[k]);
}

// Exclusive scan of per-sentence token counts -> tok_offsets (single workgroup;
// n is at most a few million per batch).
// It is also the last reader of the launch's Control block: it publishes the block to the
// pinned host copy (no D2H copy node) and zeroes the device copy for the next launch (no memset
// node) -- two operations fewer per batch on a host-launch-bound stream.
// (launched with 1024 threads behind a pool-only chain, with 256 or 64 behind a chain that holds a windowed launch: there every SIMD is full of 128-VGPR
// wavefronts, and a workgroup of sixteen wavefronts waits until a whole CU has drained -- 180 us on the chain's critical path on cfg 5, round 5)
__global__ __launch_bounds__(1024) void k_scan_counts(BatchArgs a, Control *host_ctl) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < a.n; base += nthr) {
        const uint64_t i = base + tid;
        const uint32_t v = i < a.n ? a.tok_count[i] : 0;
        const uint32_t vs = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wid] = vs;
        __syncthreads();
        uint64_t woff = 0;
        for (uint32_t w = 0; w < wid; ++w) woff += wsum[w];
        const uint64_t carry = carry_s;
        if (i < a.n) a.tok_offsets[i] = carry + woff + vs - v;
        __syncthreads();
        if (tid == nthr - 1) carry_s = carry + woff + vs;
        __syncthreads();
    }
    if (tid == 0) { a.tok_offsets[a.n] = carry_s; if (a.toff8) a.toff8[a.n] = carry_s; }   // (the mirrored table's last entry here, not in the compaction: an empty shard has no sentence to write it)
    static_assert(sizeof(Control) % 4 == 0, "Control is copied dword by dword");
    for (uint32_t k = tid; k < sizeof(Control) / 4; k += nthr) {
        uint32_t *dc = (uint32_t *)a.ctl, *hc = (uint32_t *)host_ctl;
        uint32_t v = dc[k];
        const uint32_t nt = (uint32_t)(offsetof(Control, n_tokens) / 4);
        if (k == nt) v = (uint32_t)carry_s;
        if (k == nt + 1) v = (uint32_t)(carry_s >> 32);
        __hip_atomic_store(&hc[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        dc[k] = 0;
    }
}

// Staging (dequeue order) -> dense sentence order.  One wavefront per sentence,
// dword-granular coalesced copy.
__global__ __launch_bounds__(256) void k_compact(BatchArgs a) {
    const uint32_t lane = threadIdx.x & 63, wpb = blockDim.x >> 6;   // (four wavefronts per workgroup, or one behind a chain with a windowed launch: see k_scan_counts)
    const uint64_t wave = (uint64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint32_t cnt = a.tok_count[s];
        const uint64_t dst = a.tok_offsets[s];
        if (dst + cnt > a.out_cap) continue;
        const uint32_t *src = (const uint32_t *)(a.stage + (a.offsets[s] - a.offsets[0] + s));
        uint32_t *out = (uint32_t *)(a.out + dst);
        for (uint32_t w = lane; w < cnt * 6; w += 64) out[w] = src[w];
    }
}

// Staging -> dense sentence order as 8-byte records (kgpu_token8) + the first token's (position, start) per sentence.
// One wavefront per sentence, one 8-byte store per token: when a.out8 is pinned host memory these stores are the transfer.
// (runs behind k_scan_counts, which has already published and zeroed the control block: the packing-overflow flag goes straight to the host copy)
__global__ __launch_bounds__(256) void k_compact8(BatchArgs a, Control *host_ctl) {
    const uint32_t lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * wpb;
    for (uint64_t s = wave; s < a.n; s += nwaves) {
        const uint32_t cnt = a.tok_count[s];
        const uint64_t dst = a.tok_offsets[s];
        const kgpu_token *src = a.stage + (a.offsets[s] - a.offsets[0] + s);
        if (lane == 0) {
            const uint2 f = cnt ? make_uint2(src[0].position, src[0].start) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            *(uint2 *)(a.first8 + 2 * s) = f;
            if (a.status8) a.status8[s] = a.status[s];
            if (a.toff8) a.toff8[s] = dst;   // ([n] comes from k_scan_counts)
        }
        if (dst + cnt > a.out_cap) continue;
        bool bad = false;
        for (uint32_t k = lane; k < cnt; k += 64) {
            const kgpu_token t = src[k];
            const uint32_t chars = t.end - t.start;
            bad |= chars > 0xFFFu || t.byte_len > 0x3FFFFu;
            *(uint2 *)(a.out8 + dst + k) = make_uint2((uint32_t)t.id, t.cls | (chars << 2) | (t.byte_len << 14));
        }
        if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&host_ctl->pack_overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Scan + compaction in ONE launch (batches of up to 65 536 sentences): workgroup w owns `per_wg` consecutive sentences; it sums the token counts in
// front of them itself (a few KB of L2 reads) instead of waiting for a scan kernel -- whose single 1024-thread workgroup had to find a CU with
// sixteen free wavefront slots on a chip full of pool-kernel wavefronts (8.5 us per batch, a second launch on the stream).  The LAST workgroup knows
// the total: it writes tok_offsets[n], publishes the control block to the host copy and zeroes the device copy (every field but pack_overflow, which
// this kernel's workgroups set in the host copy directly; the host clears it before the launch).
template <bool REC8>
__global__ __launch_bounds__(256) void k_scan_compact(BatchArgs a, Control *host_ctl, uint32_t per_wg) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t loff[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint64_t s0 = (uint64_t)blockIdx.x * per_wg;
    uint64_t part = 0;
    for (uint64_t i = tid; i < s0; i += 256) part += a.tok_count[i];
    part = wave_sum64(part);
    if (lane == 0) wsum[wid] = part;
    __syncthreads();
    const uint64_t prefix = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    const uint64_t si = s0 + tid;
    const uint32_t v = (tid < per_wg && si < a.n) ? a.tok_count[si] : 0u;
    const uint32_t vs = wave_incl_scan(v, lane);
    if (lane == 63) wsum[wid] = vs;
    __syncthreads();
    uint64_t woff = 0;
    for (uint32_t w = 0; w < wid; ++w) woff += wsum[w];
    const uint64_t mine = prefix + woff + vs - v;
    loff[tid] = mine;
    if (tid < per_wg && si < a.n) a.tok_offsets[si] = mine;
    const bool last_wg = s0 + per_wg >= a.n;
    const uint64_t total = prefix + wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (last_wg) {
        if (tid == 0) { a.tok_offsets[a.n] = total; if (a.toff8) a.toff8[a.n] = total; }   // (n = 0 included: an empty shard's mirrored table is {0})
        static_assert(sizeof(Control) % 4 == 0 && sizeof(Control) / 4 <= 256 * 4, "Control is copied a few dwords per thread");
        for (uint32_t k = tid; k < sizeof(Control) / 4; k += 256) {
            uint32_t *dc = (uint32_t *)a.ctl, *hc = (uint32_t *)host_ctl;
            uint32_t x = dc[k];
            const uint32_t nt = (uint32_t)(offsetof(Control, n_tokens) / 4);
            if (k == nt) x = (uint32_t)total;
            if (k == nt + 1) x = (uint32_t)(total >> 32);
            if (k != (uint32_t)(offsetof(Control, pack_overflow) / 4)) __hip_atomic_store(&hc[k], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            dc[k] = 0;
        }
    }
    __syncthreads();
    for (uint32_t t = wid; t < per_wg; t += 4) {   // one wavefront per sentence
        const uint64_t sx = s0 + t;
        if (sx >= a.n) break;
        const uint64_t dst = loff[t];
        const uint64_t nxt = t + 1 < 256 ? loff[t + 1] : total;  // (threads past the workgroup's sentences scanned zeros)
        const uint32_t cnt = (uint32_t)(nxt - dst);
        const kgpu_token *src = a.stage + (a.offsets[sx] - a.offsets[0] + sx);
        if constexpr (REC8) {
            if (lane == 0) {
                const uint2 f = cnt ? make_uint2(src[0].position, src[0].start) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
                *(uint2 *)(a.first8 + 2 * sx) = f;
                if (a.status8) a.status8[sx] = a.status[sx];
                if (a.toff8) a.toff8[sx] = dst;
            }
            if (dst + cnt > a.out_cap) continue;
            bool bad = false;
            for (uint32_t k = lane; k < cnt; k += 64) {
                const kgpu_token tk = src[k];
                const uint32_t chars = tk.end - tk.start;
                bad |= chars > 0xFFFu || tk.byte_len > 0x3FFFFu;
                *(uint2 *)(a.out8 + dst + k) = make_uint2((uint32_t)tk.id, tk.cls | (chars << 2) | (tk.byte_len << 14));
            }
            if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&host_ctl->pack_overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            if (dst + cnt > a.out_cap) continue;
            const uint32_t *srcw = (const uint32_t *)src;
            uint32_t *out = (uint32_t *)(a.out + dst);
            for (uint32_t w = lane; w < cnt * 6; w += 64) out[w] = srcw[w];
        }
    }
}

// The control block of a launch, published by the wavefront that knows the batch's total: every dword to the pinned host copy (n_tokens from `total`;
// not pack_overflow, which the compaction's wavefronts set in the host copy directly and the host clears before the launch), the device copy zeroed.
__device__ __forceinline__ void publish_control(const BatchArgs &a, Control *host_ctl, uint64_t total, uint32_t lane) {
    static_assert(sizeof(Control) % 4 == 0, "Control is copied dword by dword");
    for (uint32_t k = lane; k < sizeof(Control) / 4; k += 64) {
        uint32_t *dc = (uint32_t *)a.ctl, *hc = (uint32_t *)host_ctl;
        uint32_t x = dc[k];
        const uint32_t nt = (uint32_t)(offsetof(Control, n_tokens) / 4);
        if (k == nt) x = (uint32_t)total;
        if (k == nt + 1) x = (uint32_t)(total >> 32);
        if (k != (uint32_t)(offsetof(Control, pack_overflow) / 4)) __hip_atomic_store(&hc[k], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        dc[k] = 0;
    }
}

// Scan + compaction in ONE launch WITHOUT LDS and without a barrier (pool-only chains of up to AUX_ONE_LAUNCH_MAX sentences: kgpu_chain.cpp).  The pool
// plan fills a CU's LDS (four 40 KB workgroups) and four of the five wavefront slots per SIMD that the pool kernel's registers allow: a workgroup that asks
// for ANY LDS -- k_scan_counts, k_scan_compact -- waits until a pool workgroup has drained, one that asks for none and has at most four wavefronts takes the
// spare slot at once.  A wavefront owns G (at most 64) consecutive sentences.  It sums the token counts in front of them itself (the pool kernel has just
// written them: L2 hits, 16-byte loads, lane-strided), scans its own G counts on the DPP network, stores their offsets and copies their records as
// k_compact / k_compact8 do.  The wavefront that owns sentence n - 1 knows the total: it writes tok_offsets[n] (and toff8[n]) and publishes the control
// block.  No wavefront waits for another.  n = 0: one wavefront that publishes {0}.
// (The toff8 stores are not reached today: launch_scan_compact keeps k_scan_compact for batches with a.toff8 -- the large host call -- until that path is
// measured with this kernel.  They are what k_scan_compact / k_compact8 write, so that the switch is the launcher's condition alone.)
template <bool REC8>
__global__ __launch_bounds__(256) void k_aux_one_launch(BatchArgs a, Control *host_ctl, uint32_t G) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t s0 = wave * G;
    if (s0 >= a.n && wave != 0) return;   // (wave-uniform; wave 0 of an empty batch stays)
    uint64_t part = 0;
    const uint4 *c4 = (const uint4 *)a.tok_count;   // (the buffer's start: 16-byte aligned)
    const uint64_t q = s0 >> 2;
#pragma unroll 4
    for (uint64_t i = lane; i < q; i += 64) { const uint4 c = c4[i]; part += (uint64_t)c.x + c.y + c.z + c.w; }
    if (4 * q + lane < s0) part += a.tok_count[4 * q + lane];
    const uint64_t prefix = wave_sum64(part);
    const uint64_t si = s0 + lane;
    const bool mine = lane < G && si < a.n;
    const uint32_t v = mine ? a.tok_count[si] : 0u;
    const uint64_t slot = mine ? a.offsets[si] - a.offsets[0] + si : 0u;   // the sentence's first staging slot
    const uint32_t vs = wave_incl_scan(v, lane);
    const uint64_t off = prefix + vs - v;
    if (mine) a.tok_offsets[si] = off;
    if (s0 + G >= a.n) {   // the batch's last sentence is this wavefront's
        const uint64_t total = prefix + (uint32_t)__builtin_amdgcn_readlane((int)vs, 63);
        if (lane == 0) { a.tok_offsets[a.n] = total; if (a.toff8) a.toff8[a.n] = total; }
        publish_control(a, host_ctl, total, lane);
    }
    for (uint32_t t = 0; t < G && s0 + t < a.n; ++t) {
        const uint64_t sx = s0 + t;
        const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)t);
        const uint64_t dst = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(off >> 32), (int)t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, (int)t);
        const uint64_t sl = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(slot >> 32), (int)t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)slot, (int)t);
        const kgpu_token *src = a.stage + sl;
        if constexpr (REC8) {
            if (lane == 0) {
                const uint2 f = cnt ? make_uint2(src[0].position, src[0].start) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
                *(uint2 *)(a.first8 + 2 * sx) = f;
                if (a.status8) a.status8[sx] = a.status[sx];
                if (a.toff8) a.toff8[sx] = dst;
            }
            if (dst + cnt > a.out_cap) continue;
            bool bad = false;
            for (uint32_t k = lane; k < cnt; k += 64) {
                const kgpu_token tk = src[k];
                const uint32_t chars = tk.end - tk.start;
                bad |= chars > 0xFFFu || tk.byte_len > 0x3FFFFu;
                *(uint2 *)(a.out8 + dst + k) = make_uint2((uint32_t)tk.id, tk.cls | (chars << 2) | (tk.byte_len << 14));
            }
            if (__ballot(bad) != 0 && lane == 0) __hip_atomic_store(&host_ctl->pack_overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            if (dst + cnt > a.out_cap) continue;
            const uint32_t *srcw = (const uint32_t *)src;
            uint32_t *out = (uint32_t *)(a.out + dst);
            for (uint32_t w = lane; w < cnt * 6; w += 64) out[w] = srcw[w];
        }
    }
}

// k_scan_counts without LDS: ONE wavefront, behind a chain with small_scan (a chip full of windowed workgroups has no free LDS either: cfg 3, seven
// interleaved pairs: 33.7-34.3 -> 34.5-34.6 M sentences/s in batches of 65 536; 16.2-16.7 -> 16.6-17.1 in batches of 4096, above in each pair, the ranges overlap; behind a pool-only chain it is level with k_scan_counts or below).  A round covers 4096 counts: each lane sums 64 consecutive ones (sixteen 16-byte
// loads issued together), the lane totals are scanned on the DPP network, the lane writes its 64 offsets; the carry goes from round to round in a register.
__global__ __launch_bounds__(64) void k_scan_counts_wave(BatchArgs a, Control *host_ctl) {
    const uint32_t lane = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < a.n; base += 4096) {
        const uint64_t i0 = base + 64u * lane;
        uint32_t c[64];
        if (i0 + 64 <= a.n) {
            const uint4 *c4 = (const uint4 *)(a.tok_count + i0);
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) { const uint4 x = c4[k]; c[4 * k] = x.x; c[4 * k + 1] = x.y; c[4 * k + 2] = x.z; c[4 * k + 3] = x.w; }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 64; ++k) c[k] = i0 + k < a.n ? a.tok_count[i0 + k] : 0u;
        }
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) sum += c[k];
        const uint64_t vs = wave_incl_scan64(sum, lane);
        uint64_t o = carry + vs - sum;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) { if (i0 + k < a.n) a.tok_offsets[i0 + k] = o; o += c[k]; }
        carry += lane63(vs);
    }
    if (lane == 0) { a.tok_offsets[a.n] = carry; if (a.toff8) a.toff8[a.n] = carry; }
    publish_control(a, host_ctl, carry, lane);
}

int launch_tokenize_pool(const DictView &d, const BatchArgs &a, const WorkIO &io, uint32_t pool_bytes, uint32_t waves,
                         uint32_t max_pages, int n_workgroups, uint32_t stop_after, void *stream);  // kgpu_pool.hip
int launch_tokenize_window(const DictView &d, const BatchArgs &a, const WorkIO &io, uint32_t lds_bytes, int n_workgroups, bool team, bool claim, void *stream);  // kgpu_window.hip

// One launch of a chain (kgpu_chain.h): a persistent grid over its work list that pushes what it does not serve onto the next one.
int launch_step(const DictView &d, const BatchArgs &a, const Step &s, uint32_t stop_after, void *stream) {
    Control *ctl = a.ctl;
    const WorkIO io{s.in >= 0 ? a.ovf[s.in] : nullptr, s.in >= 0 ? &ctl->ovf_count[s.in] : nullptr, s.out >= 0 ? a.ovf[s.out] : nullptr,
                    s.out >= 0 ? &ctl->ovf_count[s.out] : nullptr, s.kernel == Kernel::Pool ? &ctl->late_count[s.out] : nullptr};
    switch (s.kernel) {
    case Kernel::Pool: return launch_tokenize_pool(d, a, io, s.lds_bytes, s.waves, s.max_pages, s.grid, stop_after, stream);
    case Kernel::WindowTeam: return launch_tokenize_window(d, a, io, s.lds_bytes, s.grid, true, false, stream);
    case Kernel::Window: return launch_tokenize_window(d, a, io, s.lds_bytes, s.grid, false, s.claim, stream);
    case Kernel::General: hipLaunchKernelGGL(k_tokenize_general, dim3((unsigned)s.grid), dim3(64), 0, (hipStream_t)stream, d, a, io, stop_after); break;
    }
    return (int)hipGetLastError();
}

int launch_small_call(const DictView &d, const BatchArgs &a, void *stream) {
    Control *ctl = a.ctl;
    WorkIO io{nullptr, nullptr, a.ovf[0], &ctl->ovf_count[0], &ctl->late_count[0]};
    // every wavefront gets at most one sentence -- and a workgroup of its own with a 64 KB LDS slice (at most 128 of them: the chip has room): no pages to
    // reserve, no wavefronts that start only to find nothing and meet at the barrier (one sentence: 52 -> 44.5 us per call, 64: 65.7 -> 57.3; round 6),
    // and anything up to ~350 characters stays in this one launch.
    return launch_tokenize_pool(d, a, io, 64u * 1024u, 1u, 64u, (int)(a.n ? a.n : 1), 0u, stream);
}
int launch_general_only(const DictView &d, const BatchArgs &a, void *stream) {
    WorkIO io{nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_tokenize_general, dim3(1), dim3(64), 0, (hipStream_t)stream, d, a, io, 0u);
    return (int)hipGetLastError();
}

int launch_general_keep(const DictView &d, const BatchArgs &a, void *stream) {
    WorkIO io{nullptr, nullptr, nullptr, nullptr, nullptr};
    const unsigned grid = (unsigned)(a.n < 1 ? 1 : a.n > 4096 ? 4096 : a.n);   // one wavefront a sentence, grid-stride beyond
    hipLaunchKernelGGL(k_tokenize_general, dim3(grid), dim3(64), 0, (hipStream_t)stream, d, a, io, 0u);
    return (int)hipGetLastError();
}

#ifndef KGPU_AUX_G
#define KGPU_AUX_G 4   // sentences per wavefront of k_aux_one_launch up to 4096 sentences (make NAME=g8 EXTRA=-DKGPU_AUX_G=8: A/B runs only)
#endif
// one_launch: what the batch's chain decided (Chain::aux_one_launch); mode: KGPU_AUX_LAUNCH (measurement / test only) -- 0 two launches, 1 one launch
// whatever the chain says (batches of up to 65 536 sentences), 2 two launches with the single-wavefront scan, anything else: by the chain (one launch where it
// asks for it; otherwise two, the single-wavefront scan where the chain asks for small workgroups).  0 is what ran before the one launch existed.
// *form: what was launched (kgpu_debug_aux_form: the tests' witness) -- 1 k_aux_one_launch, 2 k_scan_compact, 3 k_scan_counts + compaction, 4 k_scan_counts_wave + compaction.
int launch_scan_compact(const BatchArgs &a, Control *host_ctl, void *stream, bool small_workgroups, bool one_launch, int mode, int *form) {
    // Measured (tools/ab_scan.sh): records bound for mapped host memory (the large host call: a.toff8) 83.8 against 66.6 M sentences/s end to end in one
    // launch; the device-resident 24-byte path 92.8 against 96.9 -- there the separate kernels stay.
    if (!a.toff8 && a.n <= 65536 && (mode == 1 || (one_launch && mode != 0 && mode != 2))) {
        // G sentences per wavefront: four up to 4096 sentences (1024 wavefronts, a prefix of 2048 counts on average; eight, this kernel built
        // with -DKGPU_AUX_G=8: 134.7-136.2 M sentences/s on cfg 2 where four gave 137.6-139.3 and the two launches 131.5-136.0), then as many as keep the grid
        // there (forced runs only: the chain asks for one launch up to 4096 sentences) -- the prefix reads grow as n * n / G.  Workgroups of four wavefronts
        // (one per SIMD: the pool plan's spare slot), one where a windowed launch fills the chip.  profiles/experiments/aux_one_launch.txt
        uint32_t G = KGPU_AUX_G;
        *form = 1;
        while (G < 64 && (uint64_t)G * 1024 < a.n) G *= 2;
        const uint64_t waves = a.n ? (a.n + G - 1) / G : 1, wpb = small_workgroups || waves < 4 ? 1 : 4;
        const unsigned wgs = (unsigned)((waves + wpb - 1) / wpb);
        if (a.out8) hipLaunchKernelGGL(k_aux_one_launch<true>, dim3(wgs), dim3((unsigned)(64 * wpb)), 0, (hipStream_t)stream, a, host_ctl, G);
        else hipLaunchKernelGGL(k_aux_one_launch<false>, dim3(wgs), dim3((unsigned)(64 * wpb)), 0, (hipStream_t)stream, a, host_ctl, G);
        return (int)hipGetLastError();
    }
    if (a.n <= 65536 && a.toff8) {
        *form = 2;
        const uint32_t per_wg = a.n <= 4096 ? 64u : a.n <= 16384 ? 128u : 256u;
        const uint64_t wgs = a.n ? (a.n + per_wg - 1) / per_wg : 1;
        if (a.out8) hipLaunchKernelGGL(k_scan_compact<true>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, a, host_ctl, per_wg);
        else hipLaunchKernelGGL(k_scan_compact<false>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, a, host_ctl, per_wg);
        return (int)hipGetLastError();
    }
    // small_workgroups: behind a chain that holds a windowed launch the chip is full of single-wavefront workgroups at four 128-VGPR wavefronts per SIMD -- a
    // workgroup of one wavefront finds a place as soon as ANY of them ends, one of sixteen (or four) needs a CU (or a SIMD row) to drain
    const unsigned scan_threads = !small_workgroups ? 1024u : a.n > 1024 ? 256u : 64u, wpb = small_workgroups ? 1u : 4u;
    const bool wave_scan = mode == 2 || (small_workgroups && mode != 0);
    *form = wave_scan ? 4 : 3;
    if (wave_scan) hipLaunchKernelGGL(k_scan_counts_wave, dim3(1), dim3(64), 0, (hipStream_t)stream, a, host_ctl);
    else hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(scan_threads), 0, (hipStream_t)stream, a, host_ctl);
    uint64_t blocks = (a.n + wpb - 1) / wpb;
    if (blocks > 2048 * (4 / wpb)) blocks = 2048 * (4 / wpb);
    if (blocks == 0) blocks = 1;
    // (measured: the compaction of 8-byte records into mapped host memory on a stream of its own, behind an event -- so that the context's
    // stream goes on with the next batch -- gives 46.8 instead of 68.6 M sentences/s end to end: one more stream than hardware queues)
    if (a.out8) hipLaunchKernelGGL(k_compact8, dim3((unsigned)blocks), dim3(64 * wpb), 0, (hipStream_t)stream, a, host_ctl);
    else hipLaunchKernelGGL(k_compact, dim3((unsigned)blocks), dim3(64 * wpb), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace kgpu
