// kanpyo_amd/csrc/kgpu_lattice_call.h -- the one frame of the host calls that decode over kept lattices ("The kept-lattice protocol"):
// kgpu_graphviz_batch (kgpu_graphviz_host.cpp), kgpu_tokenize_batch_nbest (kgpu_nbest_batch.cpp), kgpu_tokenize_batch_marginals / _samples
// (kgpu_prob_batch.cpp), kgpu_tokenize_batch_mode (kgpu_mode_batch.cpp), kgpu_tokenize_batch_user (kgpu_user_batch.cpp).
//
// Owns: the call's common checks and the lease of ONE pooled context (the chunks run one after the other: not a throughput path); the chunks, cut by input
// bytes and sentences so that what a chunk keeps in the arena stays bounded; a chunk's launches -- the general kernel with BatchArgs::keep_lattice over the
// whole chunk, then the call's measure launches, one host wait, its write launch -- the arena_overflow protocol of the kept lattices and whatever the call
// keeps behind them; the totals against the caller's capacities; the delivery of the status bytes, and the running totals.  A call supplies an Ops type
// (a template parameter: no virtual calls, no callback tables) with what is its own:
//
//   who, hook               its name in messages (a member), its slot of the test hooks (a constant)
//   measure_what            what its measure launch is called in an error message
//   after_batch_check(d), after_length_check(d)   further checks in the places the call always had them (LatticeOps: none)
//   begin()                 the caller's offsets [0] = 0, once the context is leased
//   chunk_words(m)          the 8-byte words of the per-chunk array block (kgpu_ctx::lat_words) m sentences need
//   fill(f)                 its launch arguments from the chunk's common fields (LatticeChunk), output pointers null
//   measure(stream)         its launches up to the scan(s); -> a hipError_t as int
//   totals(t)               the device addresses of its one or two totals (t[1] null: one), final behind measure()
//   fits(done, sizes)       the totals so far plus this chunk's still fit the caller's capacities
//   out_bytes(sizes), place(block, sizes)   the size of its output block (kgpu_ctx::lat_out) for these totals, and the layout put into the arguments
//   write(stream)           its write launch
//   deliver(f, done, sizes, fits, what)     its D2H copies on f.stream (-> hipError_t; `what` names a failed one), and ...
//   fix_up(f, done, sizes, fits)            ... once they are through, the caller's offsets.  fits: nothing has overflowed so far, the write launch ran
//   report(done), too_small(done)           the caller's totals; the error text of KGPU_ERR_CAPACITY
#pragma once
#include <cstring>
#include <vector>

#include "kgpu_runtime.h"

namespace kgpu {

constexpr uint64_t LATTICE_CHUNK_BYTES = 256u << 10, LATTICE_CHUNK_SENTS = 1024;   // a chunk's input: its lattices take a few hundred bytes per input byte, and a
                                                                                   // call keeps 8 to 8 k bytes per node behind them (k paths: N-best)

// What a chunk's launches share: sentences [lo, lo + m) of the call, as they lie on the device.
struct LatticeChunk {
    uint64_t lo, m;
    const uint8_t *utf8; const uint64_t *offsets;   // the chunk's text and its m + 1 offsets from 0
    Control *ctl; uint8_t *arena; uint64_t arena_bytes; unsigned long long *desc;   // as the lattice launch has them (BatchArgs)
    const int16_t *conn; uint32_t conn_rows;
    uint8_t *status;                               // m
    uint64_t *words;                               // chunk_words(m) 8-byte words
    hipStream_t stream;
};
struct LatticeOps {   // what most calls leave as it is
    int after_batch_check(kgpu_dict *) { return KGPU_OK; }
    int after_length_check(kgpu_dict *) { return KGPU_OK; }
};
inline hipError_t d2h(void *dst, const void *src, size_t bytes, hipStream_t stream) {   // (nothing to copy is no call)
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess;
}

template <class Ops>
struct LatticeCall {
    Ops &ops;
    kgpu_dict *d; const uint8_t *utf8; const uint64_t *offsets; uint8_t *status;
    kgpu_ctx *c = nullptr;
    uint64_t done[2] = {0, 0};   // what has been delivered (or, after an overflow, counted): the call's one or two totals
    bool overflow = false;
    std::vector<uint64_t> rel;
    std::vector<uint8_t> st;
    LatticeCall(Ops &ops_, kgpu_dict *d_, const uint8_t *utf8_, const uint64_t *offsets_, uint8_t *status_) : ops(ops_), d(d_), utf8(utf8_), offsets(offsets_), status(status_) {}

    int hip_fail(hipError_t e, const char *what) {
        set_error("%s: %s: %s", ops.who, what, hipGetErrorString(e));
        c->ctl_dirty = true;
        return KGPU_ERR_HIP;
    }

    // Sentences [lo, lo + m) of the call: lattices, the call's own passes, delivery behind what has been delivered.
    int run_chunk(uint64_t lo, uint64_t m) {
        const uint64_t *off = offsets + lo;
        const uint64_t base = off[0], total = off[m] - base;
        const size_t desc_bytes = (size_t)m * LAT_DESC_WORDS * 8 + 8;
        int rc;
        // (the order of the allocations is part of the frame: run_chunks has the measurement that it matters)
        if ((rc = c->arena.ensure(ARENA_INITIAL)) || (rc = c->stage.ensure((size_t)token_bound(total, m) * sizeof(kgpu_token) + 64)) ||
            (rc = c->tok_count.ensure((size_t)m * 4 + 8)) || (rc = c->in_utf8.ensure((size_t)total + 16)) || (rc = c->in_off.ensure((size_t)(m + 1) * 8)) ||
            (rc = c->out_status.ensure((size_t)m + 16)) || (rc = c->lat_desc.ensure(desc_bytes)) || (rc = c->lat_words.ensure(ops.chunk_words(m) * 8)))
            return rc;
        rel.resize((size_t)m + 1);
        for (uint64_t i = 0; i <= m; ++i) rel[(size_t)i] = off[i] - base;
        hipError_t e;
        // (every copy and launch goes on c->stream and is waited for below: no batch is begun -- as kgpu_lattice_dump)
        if (total && (e = hipMemcpyAsync(c->in_utf8.p, utf8 + base, (size_t)total, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(e, "H2D");
        if ((e = hipMemcpyAsync(c->in_off.p, rel.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return hip_fail(e, "H2D");
        LatticeChunk f{};
        uint64_t sizes[2] = {0, 0};   // the chunk's totals
        const LatticeHooks hooks = test_hooks().lattice[Ops::hook];
        const size_t arena_max = hooks.arena_max ? (size_t)hooks.arena_max : ARENA_MAX;
        size_t limit = (size_t)hooks.arena_initial;   // what of the arena the kept lattices and what lies behind them may use (0: all of it)
        for (;;) {
            BatchArgs a{};
            a.utf8 = (const uint8_t *)c->in_utf8.p; a.offsets = (const uint64_t *)c->in_off.p; a.n = m; a.ctl = c->d_ctl;
            a.arena = (uint8_t *)c->arena.p; a.arena_bytes = arena_share(limit, c->arena.bytes);
            a.stage = (kgpu_token *)c->stage.p; a.tok_count = (uint32_t *)c->tok_count.p; a.status = (uint8_t *)c->out_status.p;
            a.keep_lattice = 1; a.lat_desc = (unsigned long long *)c->lat_desc.p;
            f = LatticeChunk{lo, m, a.utf8, a.offsets, a.ctl, a.arena, a.arena_bytes, a.lat_desc, d->view.conn, d->view.conn_rows, a.status, (uint64_t *)c->lat_words.p, c->stream};
            ops.fill(f);
            c->ctl_dirty = true;   // no scan kernel behind this launch: the next batch zeroes the block itself
            Control hc{};
            const uint64_t *t[2] = {nullptr, nullptr};
            ops.totals(t);
            if ((e = hipMemsetAsync(c->d_ctl, 0, sizeof(Control), c->stream)) != hipSuccess ||
                (e = hipMemsetAsync(c->lat_desc.p, 0, desc_bytes, c->stream)) != hipSuccess) return hip_fail(e, "memset");
            if ((e = (hipError_t)launch_general_keep(d->view, a, c->stream)) != hipSuccess) return hip_fail(e, "lattice launch");
            if ((e = (hipError_t)ops.measure(c->stream)) != hipSuccess) return hip_fail(e, Ops::measure_what);
            if ((e = hipMemcpyAsync(&hc, c->d_ctl, sizeof(Control), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                (e = hipMemcpyAsync(&sizes[0], t[0], 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                (t[1] && (e = hipMemcpyAsync(&sizes[1], t[1], 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)) return hip_fail(e, "D2H");
            if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(e, "sync");
            if (!hc.arena_overflow) break;
            // the kept lattices and what the call keeps behind them did not fit (the arena_overflow protocol, kgpu_chunk_policy.h): a bigger arena and the chunk
            // once more; at the largest arena the chunk in halves; a sentence that alone does not fit keeps KGPU_SENT_NO_SCRATCH and gives nothing
            const ArenaDecision next = arena_step(limit, c->arena.bytes, arena_max, m);
            if (next.step == ArenaStep::GROW) { if ((rc = c->arena.ensure(next.want))) return rc; if (limit) limit = next.want; c->rt.arena_regrows++; continue; }
            if (next.step == ArenaStep::HALVE) { if ((rc = run_chunk(lo, m / 2))) return rc; return run_chunk(lo + m / 2, m - m / 2); }
            break;
        }
        if (!ops.fits(done, sizes)) overflow = true;   // (from here on the chunks are only counted)
        if (!overflow) {
            if ((rc = c->lat_out.ensure(ops.out_bytes(sizes) + 16))) return rc;
            ops.place((uint8_t *)c->lat_out.p, sizes);
            if ((e = (hipError_t)ops.write(c->stream)) != hipSuccess) return hip_fail(e, "write launch");
        }
        const char *what = "D2H";
        if ((e = ops.deliver(f, done, sizes, !overflow, what)) != hipSuccess) return hip_fail(e, what);
        st.resize((size_t)m + 1);
        if (status && (e = d2h(st.data(), c->out_status.p, (size_t)m, c->stream)) != hipSuccess) return hip_fail(e, "D2H status");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(e, "sync");
        ops.fix_up(f, done, sizes, !overflow);
        if (status && m) std::memcpy(status + lo, st.data(), (size_t)m);
        done[0] += sizes[0]; done[1] += sizes[1];
        return KGPU_OK;
    }

    // The call behind its own argument checks.
    int run(uint64_t n) {
        int rc;
        if ((rc = check_host_batch(ops.who, offsets, n, utf8)) || (rc = ops.after_batch_check(d))) return rc;
        for (uint64_t i = 0; i < n; ++i)
            if (offsets[i + 1] - offsets[i] >= (1ull << 31)) { set_error("%s: sentence %llu too long", ops.who, (unsigned long long)i); return KGPU_ERR_INVALID_ARG; }
        if ((rc = ops.after_length_check(d))) return rc;
        HIPCHECK(hipSetDevice(d->device));
        PooledCtx lease(d);
        if (lease.rc) return lease.rc;
        c = lease.c;
        if (c->pending && (rc = kgpu_ctx_sync(c, nullptr)) != KGPU_OK && rc != KGPU_ERR_CAPACITY) return rc;
        rc = KGPU_OK;
        ops.begin();
        const uint64_t hook = test_hooks().lattice[Ops::hook].chunk_sents, max_sents = hook ? hook : LATTICE_CHUNK_SENTS;
        for (uint64_t at = 0; !rc && at < n;) {
            const uint64_t m = cut_chunk(offsets, at, n, max_sents, LATTICE_CHUNK_BYTES);
            rc = run_chunk(at, m);
            at += m;
        }
        ops.report(done);
        if (!rc && overflow) { ops.too_small(done); return KGPU_ERR_CAPACITY; }
        return rc;
    }
};

template <class Ops>
int lattice_call(Ops &ops, kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint8_t *status) {
    return LatticeCall<Ops>(ops, d, utf8, offsets, status).run(n);
}

}  // namespace kgpu
