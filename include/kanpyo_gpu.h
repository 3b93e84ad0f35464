/*
 * include/kanpyo_gpu.h -- C ABI of libkanpyo_gpu.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of togatoga/kanpyo: Tokenizer::tokenize()
 * (lattice build over the double-array trie + Viterbi over the connection
 * matrix).  The reference has no FFI of its own (pure safe Rust); these are the
 * entry points a Rust `kanpyo::Tokenizer` shim binds with `extern "C"` (the
 * binding is shown in INTEGRATION.md).  Each entry point cites the reference
 * interface it replaces; paths are relative to the reference checkout.
 *
 * Plain pointers and sizes only; no torch / HIP types in the signatures (a HIP
 * stream crosses as void*).  All functions return KGPU_OK (0) or a KGPU_ERR_*
 * code and never abort; kgpu_last_error() gives the thread-local message.
 */
#ifndef KANPYO_GPU_H
#define KANPYO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGPU_OK 0
#define KGPU_ERR_INVALID_ARG 1 /* null pointer, offsets not monotone, ...                */
#define KGPU_ERR_BAD_DICT 2    /* truncated blob, or a dictionary on which the reference
                                  itself would panic (index out of bounds)               */
#define KGPU_ERR_HIP 3         /* HIP runtime error (message has the hipError string)    */
#define KGPU_ERR_CAPACITY 4    /* caller's token buffer too small; *n_tokens = needed    */
#define KGPU_ERR_NO_DEVICE 5   /* no usable gfx950 device / extension built without one  */
#define KGPU_ERR_INTERNAL 6

/* Per-sentence status (uint8). */
#define KGPU_SENT_OK 0
#define KGPU_SENT_INVALID_UTF8 1 /* Rust's &str cannot carry this; the C boundary checks
                                    (reference src/tokenizer.rs:16 takes &str).  The
                                    sentence yields zero tokens.                        */
#define KGPU_SENT_NO_SCRATCH 2   /* transient: the lattice did not fit the scratch arena;
                                    kgpu_ctx_sync grows it and reruns the batch, callers
                                    never see this value                                 */
#define KGPU_SENT_TRUNCATED 3    /* measurement mode only (kgpu_ctx_set_ablation): the
                                    sentence was stopped after a stage, zero tokens      */

/* TokenClass (reference src/token.rs:3-8). */
#define KGPU_CLASS_DUMMY 0
#define KGPU_CLASS_KNOWN 1
#define KGPU_CLASS_UNKNOWN 2

/* Token (reference src/token.rs:10-18) as a fixed 24-byte record.  `surface`
 * is not materialised: it is input[position .. position + byte_len] of the
 * sentence, or the literal "EOS" when cls == KGPU_CLASS_DUMMY (byte_len == 0,
 * end == start + 3 because "EOS".chars().count() == 3, src/tokenizer.rs:28,34). */
typedef struct kgpu_token {
    int32_t id;        /* Token.id (KeywordID; 0 for the EOS dummy)      */
    uint32_t cls;      /* Token.class                                     */
    uint32_t position; /* Token.position: byte offset inside the sentence */
    uint32_t start;    /* Token.start: char index                         */
    uint32_t end;      /* Token.end: char index                           */
    uint32_t byte_len; /* surface length in bytes                         */
} kgpu_token;

/* The same Token in 8 bytes, for moving results over PCIe / xGMI (a third of the volume): consecutive tokens of a
 * sentence tile it (a path through the lattice: each word starts where the previous one ends, src/lattice.rs:144-153),
 * so position and start are running sums over the sentence and need not travel:
 *   packed = cls | chars << 2 | byte_len << 14     (chars = end - start, 12 bits; byte_len 18 bits; EOS: chars 3, byte_len 0)
 * plus, per sentence, the first token's (position, start) -- not always (0, 0): when the best chain starts at an
 * unreachable node that node is dropped (src/lattice.rs:144-153).  kgpu_expand_tokens restores
 * the 24-byte records exactly. */
typedef struct kgpu_token8 {
    int32_t id;
    uint32_t packed;
} kgpu_token8;
#define KGPU_T8_CLS(p) ((p) & 3u)
#define KGPU_T8_CHARS(p) (((p) >> 2) & 0xFFFu)
#define KGPU_T8_BYTES(p) ((p) >> 14)

/* The dictionary tables exactly as the reference serialises them
 * (DictReadWrite::write_dict, kanpyo-dict/src/dict.rs:13-18): the hot-path
 * table internals are private in the reference (trie/da.rs:14-20,
 * index.rs:10-13, connection.rs:5-9, morph.rs:24), write_dict is their only
 * public egress, so the shim hands over those bytes.
 *   index_dict      index.rs:75-84 + trie/da.rs:237-245
 *   connection_dict connection.rs:44-51
 *   morph_dict      morph.rs:61-72
 *   unk_dict        unk_dict.rs:60-73 (the trailing feature table is ignored here: kgpu_dict_set_features takes it)
 *   char_category / invoke_list / group_list: the pub Vec<u8>/Vec<bool> fields
 *                   of CharCategoryDef (char_category_def.rs:14-20), one byte each */
typedef struct kgpu_dict_blobs {
    const uint8_t *index_dict;      size_t index_len;
    const uint8_t *connection_dict; size_t connection_len;
    const uint8_t *morph_dict;      size_t morph_len;
    const uint8_t *unk_dict;        size_t unk_len;
    const uint8_t *char_category;   size_t char_category_len;
    const uint8_t *invoke_list;     size_t invoke_len;
    const uint8_t *group_list;      size_t group_len;
} kgpu_dict_blobs;

typedef struct kgpu_dict kgpu_dict; /* owns the HBM-resident tables           */
typedef struct kgpu_ctx kgpu_ctx;   /* one stream + scratch; one per thread   */

typedef struct kgpu_dict_info {
    uint64_t da_len;        /* double-array nodes (8 B each)                   */
    uint64_t n_morphs;      /* known morphs                                    */
    uint64_t n_unk_morphs;  /* unknown morphs                                  */
    uint64_t conn_rows;     /* right-id dimension                              */
    uint64_t conn_cols;     /* left-id dimension                               */
    uint64_t device_bytes;  /* HBM held by the dictionary                      */
    int32_t device;         /* HIP device ordinal                              */
    int32_t reserved;
} kgpu_dict_info;

/* Per-launch timing of the dominant kernel, collected with HIP events on the
 * ctx stream (bench.py roofline leg).  24 bytes, layout frozen: callers built against round 1 of this header
 * pass a buffer of exactly this size. */
typedef struct kgpu_profile {
    uint64_t launches;     /* tokenize kernel launches timed                  */
    double tokenize_ms;    /* sum over the timed batches of the whole tokenize launch chain (dominant kernel, long-sentence and
                              last-resort kernels, and whatever time those small launches wait for a slot on a busy chip) */
    double aux_ms;         /* sum of scan + compaction kernel durations         */
} kgpu_profile;

/* Routing counters, always on (they cost nothing: read from the batch's control block at
 * kgpu_ctx_sync).  A dictionary or text whose lattices outgrow the LDS-resident kernel shows up
 * here long before it shows up as a throughput cliff.  Read with kgpu_ctx_get_routing, which takes the
 * caller's sizeof(kgpu_routing): fields may be appended in later versions, never moved. */
typedef struct kgpu_routing {
    uint64_t batches;         /* batches completed                                            */
    uint64_t sentences;       /* sentences in them                                            */
    uint64_t deferred[4];     /* sentences handed from launch k of the chain to launch k+1
                                 ([0]: left the LDS-resident kernel for the windowed kernel;
                                 [1]: left that one for the general, HBM-scratch kernel)       */
    uint64_t redone[4];       /* ... of which only after the trie walk had been paid for
                                 (LDS reservation too small: the sentence was redone)         */
    uint64_t long_launches;   /* batches for which the windowed (long-sentence) kernel was launched */
    uint64_t arena_regrows;   /* batches rerun because the HBM scratch arena was too small    */
    double first_ms;          /* with KGPU_PROFILE_EVENTS: sum over the timed batches of the FIRST launch alone, the dominant
                                 kernel (k_tokenize_pool) -- the number rocprofv3's kernel stats report for it        */
    uint64_t small_calls;     /* kgpu_tokenize_batch calls served by the single-launch path                          */
    uint64_t small_fallbacks; /* ... that had to be redone on the general path (a sentence too long for LDS, or the
                                 in-kernel rendezvous timed out)                                                     */
    uint64_t window_reruns;   /* batches rerun with the HBM-lattice kernel because the windowed long-sentence kernel
                                 handed a sentence back                                                              */
    uint64_t tail_reruns;     /* batches whose long-sentence tail was launched afterwards (over the last work list only) because
                                 the tail of the launch chain had been left out (no recent batch needed it) and a sentence did need it */
    uint64_t combined_calls;  /* small kgpu_tokenize_batch calls that shared their launch with other threads' calls (the combiner) */
    uint64_t combined_launches; /* ... and the launches they shared                                                      */
    uint64_t window_handed[10]; /* sentences the windowed kernel handed on to the next launch, by the limit they ran into (both of its
                                 forms; of a batch rerun after the scratch arena grew (arena_regrows) the final run counts, and under [3] and [5]
                                 the sentences the runs before it flagged for want of a chunk; not counted in KGPU_PROFILE_WORK runs, whose
                                 instantiation uses the counters for its phase clocks):
                                 [0] stays 0 (a refused launch configuration and a sentence of 2^24 bytes or more are handed on uncounted)
                                 [1] a far (FIFO) entry that ends in the window has a node index more than 0x8000 below the window's base
                                 [2] more than 8 prefixes at a position and more than 48 parked in the window's shared area (also a key of
                                     256 characters or more, 255 prefixes or more at one position, 65536 records or more on one key)
                                 [3] 262144 nodes in one sentence (or a node chunk the scratch arena could not give)
                                 [4] more than 61440 far entries waiting in the FIFO
                                 [5] a far chunk the scratch arena could not give
                                 [6] far entries whose end positions decrease (a dictionary word longer than a window)
                                 [7] two-wavefront form: a carry list beyond 384 entries (both forms: a carried node index below the next window's base)
                                 [8] a window that does not fit the LDS (or its 16-bit node / slot indices) even four positions long
                                 [9] unused                                                                                       */
} kgpu_routing;

/* The launch plan a context runs with (SURVEY.md 8d cfg 5: "LDS bytes / workgroup and achieved occupancy" as data). */
typedef struct kgpu_plan_info {
    uint32_t compute_units;
    uint32_t pool_lds_bytes;          /* LDS-resident kernel: bytes of the page pool one workgroup owns            */
    uint32_t pool_wavefronts;         /* ... independent wavefronts (= sentences in flight) sharing it             */
    uint32_t pool_workgroups_per_cu;  /* ... workgroups resident per CU (occupancy API)                            */
    uint32_t pool_max_pages;          /* ... pages of 64 a sentence may take before it is routed to the long path  */
    uint32_t long_lds_bytes;          /* unused since round 4 (rounds 2-3: a second long-sentence kernel; removed) -- always 0; the three fields keep their places */
    uint32_t long_workgroups_per_cu;
    uint32_t long_workgroups;
    uint32_t window_lds_bytes;        /* windowed kernel (everything the pool kernel routes away: ~150 characters and more, any length; dense
                                         lattices): LDS per single-wavefront workgroup, 0 = off                          */
    uint32_t window_workgroups_per_cu;/* ... resident per CU (occupancy API)                                       */
    uint32_t window_workgroups;       /* ... grid of one launch                                                    */
    uint32_t streams;                 /* HIP streams the dictionary's NULL-stream contexts share: 4 when the process has GPU_MAX_HW_QUEUES >= 5
                                         (the library sets it to 16 itself when it is loaded before the HIP runtime initialises and the variable
                                         is unset), else 3 -- and kgpu_last_error() then carries a warning after kgpu_dict_create.
                                         NOTE: that setenv(GPU_MAX_HW_QUEUES=16) is PROCESS-WIDE -- it changes the hardware-queue allocation of every
                                         other HIP user in the process (PyTorch, RCCL); KGPU_NO_PREINIT=1 in the environment, or setting the variable
                                         yourself, leaves it alone (the library then runs on three shared streams, long batches included)        */
    uint32_t long_streams;            /* further streams, one per context up to this many, for batches whose chain starts with the windowed kernel
                                         (long sentences: average length >= KGPU_WINDOW_FIRST bytes, default 1024): what the hardware queues leave
                                         -- 8 with 16 queues, 2 with 8, 0 (such batches stay on `streams`) with HIP's default 4                */
    uint32_t window_first_bytes;      /* ... that threshold (0 = every chain starts with the pool kernel)                                     */
    uint32_t reserved[2];
} kgpu_plan_info;
int kgpu_ctx_get_plan(kgpu_ctx *c, kgpu_plan_info *out, size_t out_size);

/* Work counters of one or more batches, counted on the device when
 * kgpu_ctx_set_profiling(ctx, KGPU_PROFILE_WORK) is on (the
 * algorithmic-byte formulas are written in these).  Slower: not for timed runs. */
typedef struct kgpu_work {
    uint64_t sentences;
    uint64_t B; /* input bytes                                              */
    uint64_t C; /* input chars                                              */
    uint64_t T; /* double-array byte steps attempted (incl. the failing one) */
    uint64_t N; /* lattice nodes excluding BOS                              */
    uint64_t E; /* Viterbi relaxations (target, predecessor) pairs          */
    uint64_t K; /* emitted tokens                                           */
} kgpu_work;

#define KGPU_PROFILE_OFF 0
#define KGPU_PROFILE_EVENTS 1 /* HIP events around the kernels            */
#define KGPU_PROFILE_WORK 2   /* device-side work counters (kgpu_work)    */
#define KGPU_PROFILE_SAMPLED 4 /* with EVENTS: time every 4th launch only  */
#define KGPU_PROFILE_NO_T 8    /* with WORK: leave kgpu_work.T at 0 -- the byte-level walk that counts the reference's trie steps runs
                                  beside the product's character-level walk and distorts the walk phase of kgpu_ctx_get_phase_cycles */

const char *kgpu_last_error(void);
int kgpu_device_count(void);

/* Tokenizer::new(dict) (src/tokenizer.rs:12-14): parse + validate the blobs,
 * upload once to HBM of `device`.  A dictionary on which the reference would
 * panic at tokenize time (morph id / connection index / invoke_list index out
 * of bounds: src/lattice.rs:54,182,195, connection.rs:13) is rejected here with
 * KGPU_ERR_BAD_DICT instead. */
int kgpu_dict_create(const kgpu_dict_blobs *blobs, int device, kgpu_dict **out);
/* Create-time validation is stricter than the reference's lazy panics, on purpose (a device kernel
 * cannot panic): a dictionary is rejected as a whole if ANY morph carries a negative context id, if
 * the largest (left, right) id pair of the dictionary indexes outside the matrix, if a duplicate
 * count exceeds 65535 or names a missing record, or if a category that occurs in char_category has
 * no invoke_list entry -- even when the offending entry could never be reached by a lattice. */
/* The handle may be destroyed while contexts made from it are alive: the tables and the shared
 * streams are released when the last such context is destroyed. */
void kgpu_dict_destroy(kgpu_dict *d);
int kgpu_dict_get_info(const kgpu_dict *d, kgpu_dict_info *out);

/* Tokenizer::tokenize(&self, &str) -> Vec<Token> (src/tokenizer.rs:16-45) for a
 * batch of n sentences in host memory: sentence i is
 * utf8[offsets[i] .. offsets[i+1]) (offsets has n+1 entries).  Tokens are
 * written densely in sentence order; tok_offsets (n+1 entries) delimits each
 * sentence's Vec<Token>.  A sentence whose EOS is unreachable yields zero
 * tokens, as in the reference (src/lattice.rs:144-153).  status may be NULL.
 * Thread-safe per dict (&self, src/tokenizer.rs:16): each call checks a ctx
 * out of an internal pool.  token_capacity >= total_chars + n always suffices. */
int kgpu_tokenize_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                        kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets,
                        uint8_t *status, uint64_t *n_tokens);

/* The same call over several devices of one node (reference src/tokenizer.rs:16 is &self, Send + Sync: a server shards its
 * sentences; BASELINE cfg 4: "sharded round-robin"): sentence i goes to dicts[i mod n_dicts] -- one dictionary handle per device,
 * made by kgpu_dict_create on that device (the same handle may appear more than once: its device then takes several shards) --
 * one host thread per entry drives its device's chunk pipeline, every device's compaction kernel writes its 8-byte records into
 * pinned host memory, and the records are expanded into `tokens` in the caller's ORIGINAL sentence order: the result is
 * byte-for-byte what kgpu_tokenize_batch gives on one device.  No data-path collective: the shards are independent.
 * EXPERIMENTAL (this entry point and kgpu_multi_* below): exercised with one device appearing several times; never yet run with handles on two physical
 * GPUs (tests/test_gpu_multi.py::test_one_handle_per_device does as soon as a box has two).  One difference from kgpu_tokenize_batch: a token that does not
 * fit the 8-byte record the shards write (more than 4095 characters or 262143 bytes: no real dictionary) fails the whole call with KGPU_ERR_INTERNAL, where
 * the single-device call redoes that chunk with 24-byte records.  The caller's current HIP device is restored before the call returns. */
int kgpu_tokenize_batch_multi(kgpu_dict *const *dicts, int n_dicts, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                              kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, uint8_t *status, uint64_t *n_tokens);
/* ... with the records left as the devices produce them (round 6): `tokens8` receives the 8-byte kgpu_token8 records and first[2 i], first[2 i + 1] the
 * (position, start) of sentence i's first token, both in the caller's ORIGINAL sentence order; kgpu_expand_tokens(tokens8 + tok_offsets[a], tok_offsets + a,
 * first + 2 a, b - a, out) restores the 24-byte kgpu_token records of sentences [a, b) wherever and whenever the caller consumes them (or never: id, class,
 * lengths are all in the 8-byte record).  The 24-byte form's expansion writes ~1 KB of host memory per 40-character sentence on the calling side and binds
 * at about two devices' worth of records on 16 host CPUs; this form's merge moves a third of that (reference src/token.rs:10-18: a Token is id, class and
 * three positions -- the positions are running sums of the lengths).  Same sharding, same status bytes, same errors, same EXPERIMENTAL note. */
int kgpu_tokenize_batch_multi_compact(kgpu_dict *const *dicts, int n_dicts, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                      kgpu_token8 *tokens8, uint64_t token_capacity, uint32_t *first, uint64_t *tok_offsets, uint8_t *status, uint64_t *n_tokens);

/* Device-resident multi-device step with the result gather (the "trivial result gather over xGMI"): shard g -- n[g] sentences, packed
 * as kgpu_tokenize_device wants them -- is resident on dicts[g]'s device; its compaction kernel stores the 8-byte records (and the
 * per-sentence first position / start, token offsets and status bytes) straight into the ROOT device's memory through peer access
 * (root_* [g]: device pointers on dicts[0]'s device, one set per shard) -- the stores are the transfer, there is no copy node and no
 * collective.  `slot` in [0, slots): independent sets of contexts, so that several steps are in flight; kgpu_multi_sync(slot) waits
 * for that slot's shards and reports the token count of each. */
typedef struct kgpu_multi kgpu_multi;
int kgpu_multi_create(kgpu_dict *const *dicts, int n_dicts, int slots, kgpu_multi **out);
void kgpu_multi_destroy(kgpu_multi *m);
int kgpu_multi_tokenize_device(kgpu_multi *m, int slot, const uint8_t *const *d_utf8, const uint64_t *const *d_offsets, const uint64_t *n,
                               const uint64_t *total_bytes, kgpu_token8 *const *root_tokens8, const uint64_t *token_capacity,
                               uint32_t *const *root_first, uint64_t *const *root_tok_offsets, uint8_t *const *root_status);
int kgpu_multi_sync(kgpu_multi *m, int slot, uint64_t *n_tokens /* [n_dicts], may be NULL */);

/* Pinned host memory for the buffers of kgpu_tokenize_batch (optional): with it the host<->device copies of a
 * large call run as DMA and overlap the kernels of its other chunks; pageable buffers work, more slowly. */
void *kgpu_host_alloc(uint64_t bytes);
void kgpu_host_free(void *p);

/* Device-resident form (inputs already in HBM, outputs left in HBM, e.g. for
 * the RCCL gather).  All d_* pointers are device pointers on the dict's
 * device.  kgpu_tokenize_device only enqueues on the ctx stream;
 * kgpu_ctx_sync waits and reports the dense token count (or KGPU_ERR_CAPACITY). */
int kgpu_ctx_create(kgpu_dict *d, void *hip_stream /* NULL: one of the dictionary's shared streams (kgpu_plan_info.streams of them) */, kgpu_ctx **out);
/* One batch in flight per ctx; keep four or more contexts busy to fill the chip (eight for cfg 2's 4096-sentence batches).  Contexts may share a
 * stream (each waits on its own completion event); those created with NULL share kgpu_plan_info.streams per dictionary -- a NULL-stream context
 * runs each batch on the least-loaded of the dictionary's shared streams -- and a batch of long
 * sentences is moved to one of kgpu_plan_info.long_streams for its duration.  With a caller-owned stream everything stays on that stream. */
void kgpu_ctx_destroy(kgpu_ctx *c);
int kgpu_tokenize_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                         uint64_t total_bytes, kgpu_token *d_tokens, uint64_t token_capacity,
                         uint64_t *d_tok_offsets, uint8_t *d_status);
int kgpu_ctx_sync(kgpu_ctx *c, uint64_t *n_tokens);
/* Same batch, results as 8-byte records: d_tokens8 (token_capacity entries), d_first (2 n entries: position and start of
 * each sentence's first token, 0xFFFFFFFF twice for a sentence without tokens), d_tok_offsets, d_status.  The output
 * pointers may be device pointers of pinned, device-mapped host memory: the compaction kernel's stores are then the
 * device-to-host transfer.  A token that does not fit the packing (more than 4095 chars or 262143 bytes: no real
 * dictionary) makes kgpu_ctx_sync return KGPU_ERR_CAPACITY with *n_tokens = 0; use the 24-byte form for such a batch. */
int kgpu_tokenize_device_compact(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                 uint64_t total_bytes, kgpu_token8 *d_tokens8, uint64_t token_capacity,
                                 uint32_t *d_first, uint64_t *d_tok_offsets, uint8_t *d_status);
/* Host side: 8-byte records of n sentences -> the 24-byte records (running sums per sentence).  tok_offsets: n + 1
 * entries delimiting the sentences inside `in`; `out` receives tok_offsets[n] - tok_offsets[0] records. */
void kgpu_expand_tokens(const kgpu_token8 *in, const uint64_t *tok_offsets, const uint32_t *first, uint64_t n, kgpu_token *out);
int kgpu_ctx_set_profiling(kgpu_ctx *c, int mode /* KGPU_PROFILE_* bit mask */);
int kgpu_ctx_get_profile(kgpu_ctx *c, kgpu_profile *out, int reset);
/* Copies min(out_size, sizeof(kgpu_routing)) bytes: a caller built against an older, shorter kgpu_routing stays valid. */
int kgpu_ctx_get_routing(kgpu_ctx *c, kgpu_routing *out, size_t out_size, int reset);
/* The same counters summed over the dictionary's pooled contexts -- the ones kgpu_tokenize_batch and kgpu_lattice_dump check out per call (idle
 * ones only: a context serving a call right now is counted once it is back).  This is where small_calls / combined_calls show. */
int kgpu_dict_get_routing(kgpu_dict *d, kgpu_routing *out, size_t out_size, int reset);
/* Measurement only (bench.py's per-stage roofline): every sentence of the following batches stops
 * after the given stage of the fused kernel, yields zero tokens and status KGPU_SENT_TRUNCATED.
 * 0 = off (normal operation).  Stages: 5 = lattice built (SURVEY.md 8d Stage A: load, decode, trie
 * walk, numbering, node emission), 7 = Viterbi sweep done (Stage B: connection-cost gather + sweep);
 * the remainder is Stage C (backtrace + token records). */
#define KGPU_STAGE_ALL 0
#define KGPU_STAGE_LATTICE 5
#define KGPU_STAGE_GATHER 6
#define KGPU_STAGE_VITERBI 7
int kgpu_ctx_set_ablation(kgpu_ctx *c, int stop_after_stage);
int kgpu_ctx_get_work(kgpu_ctx *c, kgpu_work *out, int reset);
/* Sum over sentences of shader-clock cycles spent per phase of the LDS-resident
 * kernel (KGPU_PROFILE_WORK runs only): load, decode, walk, scan, emit, gather,
 * sweep, backtrace+tokens, [8] = sentences counted, [9] spare. */
int kgpu_ctx_get_phase_cycles(kgpu_ctx *c, uint64_t out[10], int reset);

/* Lattice (reference src/lattice.rs:6-10: pub nodes, pub edges) of ONE sentence, read back from the device after
 * Lattice::build + the forward pass of Lattice::viterbi -- the debugging aid behind the reference's `kanpyo graphviz`
 * (src/graphviz.rs:30-163, src/bin/kanpyo.rs:127-148).  Nodes are in the reference's insertion order (BOS = 0, EOS last);
 * edges[e] = the nodes ENDING at char position e, ascending, as offsets into edge_nodes (n_positions + 1 entries,
 * n_positions = chars + 2).  Context ids are the dictionary's own (not the device's frequency-ranked ones).
 * dp / pre are the Viterbi state of src/lattice.rs:118-141: dp = 1 << 30 where unreached, BOS has dp 0 ("None") and
 * pre -1.  Runs the HBM-scratch kernel alone (any sentence length); not a fast path.  Free with kgpu_lattice_free. */
typedef struct kgpu_lattice_node {
    int32_t id;          /* Node::id(): KeywordID, 0 for BOS / EOS              (src/lattice/node.rs:27-32) */
    uint32_t cls;        /* KGPU_CLASS_DUMMY / KNOWN / UNKNOWN                                              */
    uint32_t byte_pos;   /* byte offset of the surface in the sentence                                      */
    uint32_t char_pos;   /* char index where the node starts                                                */
    uint32_t end_char;   /* char index where it ends (EOS: char_pos; BOS: 0)                                */
    uint32_t byte_len;   /* surface length in bytes                                                         */
    int16_t left_id, right_id, cost, reserved; /* Morph (kanpyo-dict/src/morph.rs:7-11)                     */
    int32_t dp;          /* best total cost up to and including this node                                   */
    int32_t pre;         /* best predecessor node index, -1 = None                                          */
} kgpu_lattice_node;
typedef struct kgpu_lattice {
    uint64_t n_nodes, n_positions;
    kgpu_lattice_node *nodes;
    uint32_t *edge_offsets; /* n_positions + 1 */
    uint32_t *edge_nodes;   /* n_nodes         */
} kgpu_lattice;
int kgpu_lattice_dump(kgpu_dict *d, const uint8_t *utf8, uint64_t len, kgpu_lattice *out);
void kgpu_lattice_free(kgpu_lattice *l);

/* IndexTable::build + write_dict (kanpyo-dict/src/index.rs:16-38,75-84 over
 * trie/da.rs:22-131,191-217): sorted keywords (duplicates adjacent) -> the
 * index.dict blob, byte-identical to the reference's first-fit packing.  Host
 * only.  Free the blob with kgpu_free. */
int kgpu_index_build(const uint8_t *keys, const uint64_t *key_offsets, uint64_t n,
                     uint8_t **blob, size_t *blob_len);
void kgpu_free(void *p);

/* ---- the `kanpyo tokenize` output (reference src/bin/kanpyo.rs:106-126 tokenize, :174-197 print_tokens) ----
 * Per token one line: surface, '\t', the morph's features joined with ',', '\n'.  The surface is input[position .. position + byte_len],
 * or "EOS" for KGPU_CLASS_DUMMY; the features are empty for the dummy class and for id 0 (BOS_EOS_ID, src/lattice/node.rs:3), else
 * morph_feature_table.morph_features[id - 1] (known) or unk_dict.morph_feature_table.morph_features[id - 1] (unknown) through name_list
 * (:178-188).  A sentence without tokens (EOS unreachable, or KGPU_SENT_INVALID_UTF8) renders to 0 bytes. */

/* The display tables, in the reference's own serialised form (bincode 2, standard config: kanpyo-dict/src/morph_feature.rs:6-37):
 *   morph_feature_dict  morph_feature.dict (kanpyo-dict/src/dict.rs:58-59): dict.morph_feature_table.write_dict
 *   unk_feature_dict    the tail of unk.dict behind the morph block (unk_dict.rs:71): dict.unk_dict.morph_feature_table.write_dict
 * Trailing bytes are ignored.  KGPU_ERR_BAD_DICT wherever the reference would panic while printing: fewer rows than (unknown) morphs
 * (kanpyo.rs:178-186, morph_features[id - 1]), a feature id at or past name_list.len() in a row a token can name (:181,188; rows past the
 * morph count are never printed and not checked).  Like Dict::load, the call also fails on a truncated blob, an integer tag that does not
 * fit its type and a name that is not UTF-8.  Once per handle (a second call: KGPU_ERR_INVALID_ARG); kgpu_dict_info.device_bytes
 * grows by what is uploaded.  The lines calls below return KGPU_ERR_INVALID_ARG on a handle without them. */
int kgpu_dict_set_features(kgpu_dict *d, const uint8_t *morph_feature_dict, size_t morph_feature_len,
                           const uint8_t *unk_feature_dict, size_t unk_feature_len);
/* Tokenizer::tokenize + print_tokens for n sentences in host memory: text_offsets[i] .. text_offsets[i + 1] are sentence i's lines
 * (n + 1 entries).  status may be NULL.  KGPU_ERR_CAPACITY: *n_bytes is the exact size needed (the kgpu_tokenize_batch protocol). */
int kgpu_tokenize_batch_lines(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                              uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);
/* Device-resident: render records that a synced kgpu_tokenize_device batch (or anyone) left in HBM -- sentence i's records are
 * d_tokens[d_tok_offsets[i] .. d_tok_offsets[i + 1]) -- into d_text / d_text_offsets (n + 1); enqueued on c's stream.  kgpu_ctx_sync_lines
 * waits and reports the byte count: KGPU_ERR_CAPACITY (nothing written) when it exceeds text_capacity, KGPU_ERR_INVALID_ARG when a record
 * names a class, id or surface the dictionary or its sentence does not have. */
int kgpu_format_lines_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                             const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                             uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets);
int kgpu_ctx_sync_lines(kgpu_ctx *c, uint64_t *n_bytes);
/* Host helper: the CLI's read_line + trim_end (src/bin/kanpyo.rs:114-122) over a block of input.  Lines end at '\n' only (a final line
 * without one counts; empty input has none); each line loses its trailing Unicode White_Space (U+0009-000D, U+0020, U+0085, U+00A0,
 * U+1680, U+2000-200A, U+2028, U+2029, U+202F, U+205F, U+3000: complete encodings only, invalid bytes are kept).  The trimmed lines are
 * packed into `out` (len bytes always suffice), delimited by offsets[0 .. *n_lines] (*n_lines + 1 entries).  KGPU_ERR_CAPACITY:
 * offsets_capacity < lines + 1, *n_lines = lines. */
int kgpu_split_lines(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t *offsets, uint64_t offsets_capacity, uint64_t *n_lines);
/* read_line + trim_end (src/bin/kanpyo.rs:114-122) over a block resident in HBM; semantics of kgpu_split_lines.
 * d_out: len bytes always suffice; must not overlap d_in (KGPU_ERR_INVALID_ARG).  d_offsets: offsets_capacity entries.  len of 2^32 or
 * more is KGPU_ERR_INVALID_ARG (positions are 32-bit on the device): split the block at a '\n'.  len == 0 is valid: no lines, offsets[0] = 0.
 * Enqueued on c's stream.  kgpu_ctx_sync_split waits and reports the line count and the packed byte count;
 * KGPU_ERR_CAPACITY when n_lines + 1 > offsets_capacity (*n_lines is set; d_out / d_offsets contents unspecified). */
int kgpu_split_lines_device(kgpu_ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out,
                            uint64_t *d_offsets, uint64_t offsets_capacity);
int kgpu_ctx_sync_split(kgpu_ctx *c, uint64_t *n_lines, uint64_t *n_bytes);

/* tokenize (:106-126) over a raw block of input in HOST memory: split + trim on the device, Tokenizer::tokenize and
 * print_tokens per line; the outputs and the errors of kgpu_tokenize_batch_lines, with the line count found, not given.
 * text_offsets / status: offsets_capacity / offsets_capacity - 1 entries (status may be NULL).  n_lines and n_bytes are required.
 * KGPU_ERR_CAPACITY: *n_lines and *n_bytes are the exact sizes needed (either may be the one that did not fit). */
int kgpu_tokenize_text_lines(kgpu_dict *d, const uint8_t *text, uint64_t len,
                             uint8_t *out_text, uint64_t text_capacity, uint64_t *text_offsets, uint64_t offsets_capacity,
                             uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes);

/* ---- the `kanpyo graphviz` output (reference src/bin/kanpyo.rs:31-48,127-148 graphviz over src/graphviz.rs:30-163) ----
 * Lattice::build + the forward pass of Lattice::viterbi + Graphviz::graphviz(dpi, full_state) for n sentences in host memory, all on the
 * device: text_offsets[i] .. text_offsets[i + 1] (n + 1 entries) is sentence i's DOT document, byte for byte what the reference prints --
 * the five header lines with dpi in decimal (:36-40), one line per visible node (:55-119: every node in insertion order when full_state
 * is non-zero, else what the BFS from the last node reaches, :10-28, in the BTreeSet's order), the edge lines (:120-161) and "}".
 * Labels hold the surface, the morph's feature names without "*" joined by '/', and the cost, separated by newline bytes; nothing is
 * escaped, as in the reference.  A sentence that is not UTF-8 gets KGPU_SENT_INVALID_UTF8 and 0 bytes (status may be NULL); one whose
 * lattice does not fit the largest scratch arena gets KGPU_SENT_NO_SCRATCH and 0 bytes.  Needs kgpu_dict_set_features
 * (KGPU_ERR_INVALID_ARG without).  KGPU_ERR_CAPACITY: *n_bytes is the exact size needed (the kgpu_tokenize_batch_lines protocol; a
 * call whose input is one chunk -- up to 256 KiB and 1024 sentences -- has written nothing then).  A fixed number of launches per chunk
 * of the input, whatever it holds; the chunks run one after the other: a debugging aid for batches, not a throughput path. */
int kgpu_graphviz_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                        uint64_t dpi, int full_state,
                        uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets /* n + 1 */,
                        uint8_t *status /* may be NULL */, uint64_t *n_bytes);

/* ---- wakati-gaki: the words of each sentence on one line (NOT an output of the reference: what `mecab -Owakati` prints) ----
 * A words handle fixes a field, a filter and a separator for one dictionary, which must have its feature tables
 * (kgpu_dict_set_features).  Rendering a batch gives, for EVERY sentence, exactly one line: the words of its kept tokens joined by the
 * separator byte, then '\n'.  Line i of the output is sentence i of the input, always.
 *  1. EOS.  The EOS token (class dummy) is never a word: the line's '\n' stands for it.  A dummy record with any id, position or length
 *     (crafted records) is skipped the same way.
 *  2. Field.  KGPU_WORDS_SURFACE (-1): the word is the surface input[position .. position + byte_len).  k >= 0: the word is feature k of
 *     the token's row -- morph_features[id - 1] of the known or unknown table through name_list, the rows kgpu_tokenize_batch_lines joins
 *     (reference src/bin/kanpyo.rs:174-197).  The word FALLS BACK TO THE SURFACE when the token has no row (id 0), when the row has k
 *     features or fewer, and when feature k is the empty string or exactly "*".  IPADIC's layout, for orientation only: 0-3 part of
 *     speech, 4-5 conjugation, 6 base form, 7 reading, 8 pronunciation; unknown-word rows have 7 columns with "*" at 6.
 *  3. Filter.  `names` is a list of strings compared bytewise with feature 0 of the token's row.  KGPU_WORDS_ALL: every non-EOS token is
 *     kept, the list is ignored.  KGPU_WORDS_DROP: tokens whose feature 0 is in the list are dropped.  KGPU_WORDS_KEEP: only tokens whose
 *     feature 0 is in the list are kept.  A token without a row, or with an empty row, has no feature 0 and matches no name: DROP keeps
 *     it, KEEP drops it.  A name no row carries is not an error.  An empty list is legal: DROP with it keeps all, KEEP with it makes
 *     every line empty.
 *  4. Separator.  One byte, default ' '; '\n' is rejected.  Nothing is escaped.  An empty word is an empty word (crafted zero-length
 *     surfaces only): two separators then meet.  A token whose surface is itself a space (IPADIC's 記号,空白) is printed as it is: drop
 *     記号 if that matters.
 *  5. Sentences with no words -- no kept token, no tokens at all (EOS unreachable), KGPU_SENT_INVALID_UTF8 -- render to the single
 *     byte '\n'; the status byte is what the tokenize call reports.
 *  6. Records are range-checked as the lines render checks them (class, id within its table, surface inside the sentence): a bad record
 *     anywhere makes the sync return KGPU_ERR_INVALID_ARG. */
#define KGPU_WORDS_SURFACE (-1)
#define KGPU_WORDS_ALL 0
#define KGPU_WORDS_DROP 1
#define KGPU_WORDS_KEEP 2
typedef struct kgpu_words_spec {
    uint32_t size;                 /* sizeof(kgpu_words_spec): fields may be appended later */
    int32_t field;
    uint32_t filter;               /* KGPU_WORDS_ALL / DROP / KEEP */
    uint32_t separator;            /* one byte value, 0 = the default ' ' */
    const uint8_t *names;          /* n_names strings, concatenated ... */
    const uint64_t *name_offsets;  /* ... n_names + 1 entries */
    uint64_t n_names;
} kgpu_words_spec;
typedef struct kgpu_words kgpu_words;
/* KGPU_ERR_INVALID_ARG: a null pointer, a `size` smaller than the struct, a field below -1, an unknown filter, a separator above 255 or
 * equal to '\n', names without offsets (n_names != 0 with name_offsets NULL, or name bytes with names NULL), offsets that run backwards,
 * a dictionary without feature tables.  The handle is immutable once created: any number of threads may use it at once.  It keeps the
 * dictionary's tables alive, as a context does (it may outlive kgpu_dict_destroy).  It owns one 8-byte entry per known and unknown morph
 * and a pool of the distinct names the field selects, uploaded once (about 3 MB of entries for IPADIC) and freed by kgpu_words_destroy.
 * Host memory: kgpu_dict_set_features keeps a copy of its two blobs in the dictionary handle for this call to parse (their size, ~15 MB
 * for IPADIC, until the dictionary is released). */
int kgpu_words_create(kgpu_dict *d, const kgpu_words_spec *spec, kgpu_words **out);
void kgpu_words_destroy(kgpu_words *w);
/* kgpu_tokenize_batch_lines with the words render: text_offsets[i] .. text_offsets[i + 1] is sentence i's line (never empty: it ends with
 * '\n').  The same argument checks, the same KGPU_ERR_CAPACITY with the exact size in *n_bytes, the same status bytes. */
int kgpu_tokenize_batch_words(kgpu_words *w, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                              uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);
/* kgpu_tokenize_text_lines with the words render: a raw block of input, split and trimmed on the device, one output line per input line. */
int kgpu_tokenize_text_words(kgpu_words *w, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                             uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes);
/* kgpu_format_lines_device with the words render, enqueued on c's stream and waited for with kgpu_ctx_sync_lines (one render pending per
 * context, whichever kind).  A context whose dictionary is not the handle's: KGPU_ERR_INVALID_ARG. */
int kgpu_format_words_device(kgpu_ctx *c, const kgpu_words *w, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                             const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                             uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets);

/* ---- word counts: the frequencies of a corpus's words, accumulated on the device (NOT an output of the reference: what
 * `mecab -Owakati | tr ' ' '\n' | sort | uniq -c | sort -rn` prints) ----
 * A counts handle is made from a words handle and inherits its field and its filter; the separator plays no part.  It accumulates over any
 * number of calls until it is reset; only status bytes return from an adding call, and the read-out is as large as the vocabulary, not the input.
 *  1. Which tokens count.  Exactly the tokens wakati keeps (rules 1 and 3 above): EOS and dummy records never count; a sentence with
 *     KGPU_SENT_INVALID_UTF8, or without tokens, adds nothing.
 *  2. The word is wakati's rule 2, with one sharpening: when the word of a KNOWN token with an id (id != 0) is its surface, the word is THE
 *     DICTIONARY'S KEY OF THAT ID.  For the tokenizer's own records these are the same bytes.  For caller-made records the record's position
 *     and length are range-checked but do not choose the word.
 *  3. The key is the word's bytes.  Tokens with different ids and the same bytes are one entry (duplicate surfaces, a base form equal to
 *     another word's surface, a pool name equal to an unknown surface).  The empty word is a key (crafted zero-length surfaces of tokens that
 *     are not known-with-an-id only).  Bytes are compared as bytes: "a" and "a\0" differ.
 *  4. Counts are 64-bit.
 *  5. The read-out gives the distinct words with their counts, ordered by count descending, then by the word's bytes ascending (memcmp; a
 *     proper prefix comes first).  An optional `top` cuts the list after the sort.  The order does not depend on the order of insertion.
 *  6. Capacity.  Words that a feature row determines (a known token with an id; a name of the field) have one counter per row and always fit.
 *     All other words (unknown-class surfaces, surfaces of tokens without a row) live in a byte-keyed table of `table_slots` slots whose key
 *     bytes are copied into an arena of `key_bytes` bytes; both are fixed at create (0 selects the default: KGPU_COUNTS_DEFAULT_SLOTS = 2^22
 *     slots, 64 MiB, and KGPU_COUNTS_DEFAULT_KEY_BYTES = 256 MiB; table_slots is rounded up to a power of two; a key takes its length
 *     rounded up to 8, plus 8, and a word that several wavefronts meet for the first time at once may take that more than once).  A token
 *     whose word cannot be inserted is added to overflow_tokens and the call returns KGPU_ERR_CAPACITY -- after it has counted everything
 *     else.  The handle stays usable and consistent: every reported count is <= the true count, the reported counts and overflow_tokens sum
 *     to the tokens kept, and while overflow_tokens == 0 every count is exact.  The table does not grow.
 *  7. Bad records (wakati rule 6) make the sync return KGPU_ERR_INVALID_ARG; the handle's contents are then unspecified until it is reset.
 *  8. Threads.  Any number of threads may add into one handle at once; read-out and reset take the handle exclusively (a count enqueued on a
 *     context is synced first).  The handle keeps the words handle's tables and the dictionary alive, as a words handle keeps the dictionary:
 *     it may outlive both handles. */
#define KGPU_COUNTS_DEFAULT_SLOTS (1ull << 22)
#define KGPU_COUNTS_DEFAULT_KEY_BYTES (256ull << 20)
typedef struct kgpu_counts_opts {
    uint32_t size;         /* sizeof(kgpu_counts_opts): fields may be appended later */
    uint32_t reserved;
    uint64_t table_slots;  /* slots of the byte-keyed table (16 bytes each), 0 = the default */
    uint64_t key_bytes;    /* bytes of its key arena, 0 = the default; at most 2^34 */
} kgpu_counts_opts;
typedef struct kgpu_counts_info {
    uint32_t size;              /* in: sizeof(kgpu_counts_info) as the caller knows it; that many bytes are written at most */
    uint32_t reserved;
    uint64_t tokens_counted;    /* tokens added to a counter: the sum of all counts */
    uint64_t overflow_tokens;   /* kept tokens that found no slot or no key space */
    uint64_t sentences;         /* sentences the adding calls have seen */
    uint64_t table_slots, table_slots_used;
    uint64_t key_bytes, key_bytes_used;
} kgpu_counts_info;
typedef struct kgpu_counts kgpu_counts;
/* opts may be NULL (the defaults).  KGPU_ERR_INVALID_ARG: a null handle, an opts.size smaller than the struct, sizes beyond 2^32 slots / 2^34 bytes. */
int kgpu_counts_create(kgpu_words *w, const kgpu_counts_opts *opts, kgpu_counts **out);
void kgpu_counts_destroy(kgpu_counts *k);
int kgpu_counts_reset(kgpu_counts *k);   /* every count, overflow_tokens and sentences back to zero */
int kgpu_counts_get_info(kgpu_counts *k, kgpu_counts_info *info);
/* The sentences of kgpu_tokenize_batch_words, tokenized and counted: nothing but the status bytes (n entries, may be NULL) comes back. */
int kgpu_count_batch(kgpu_counts *k, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint8_t *status);
/* The raw block of kgpu_tokenize_text_words.  *n_lines: the lines found (required).  status (may be NULL): status_capacity entries;
 * KGPU_ERR_CAPACITY with *n_lines set and NOTHING counted when the lines outnumber them. */
int kgpu_count_text(kgpu_counts *k, const uint8_t *text, uint64_t len, uint8_t *status, uint64_t status_capacity, uint64_t *n_lines);
/* Device-resident: count records that a synced kgpu_tokenize_device batch (or anyone) left in HBM, enqueued on c's stream; kgpu_ctx_sync_count
 * waits and reports the tokens this batch added (rules 6 and 7 give its errors).  One render or count may be pending per context, whichever
 * kind.  A context whose dictionary is not the handle's: KGPU_ERR_INVALID_ARG. */
int kgpu_count_words_device(kgpu_ctx *c, kgpu_counts *k, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                            const kgpu_token *d_tokens, const uint64_t *d_tok_offsets);
int kgpu_ctx_sync_count(kgpu_ctx *c, uint64_t *n_counted);
/* The read-out of rule 5: entry i is words[word_offsets[i] .. word_offsets[i + 1]) with counts[i]; top = 0: all of them.  *n_entries and
 * *n_bytes (both required) are the exact sizes; KGPU_ERR_CAPACITY (nothing written) when entries_capacity < *n_entries or words_capacity <
 * *n_bytes.  word_offsets: entries_capacity + 1 entries, counts: entries_capacity.  Not a hot path: the counters come back to the host, every
 * row is resolved to its bytes (a name of the field, or the dictionary's key of the id), equal byte strings are merged and the list is sorted. */
int kgpu_counts_read(kgpu_counts *k, uint64_t top, uint8_t *words, uint64_t words_capacity, uint64_t *word_offsets, uint64_t *counts,
                     uint64_t entries_capacity, uint64_t *n_entries, uint64_t *n_bytes);

/* ---- vocabulary ids: sentences to int32 ids of a fixed word list, on the device (NOT an output of the reference: what a model's embedding
 * layer takes) ----
 * A vocabulary handle is made from a words handle and inherits its field and its filter; the separator plays no part.  It also takes a list
 * of n_words words (packed: word i is words[word_offsets[i] .. word_offsets[i + 1])) and a kgpu_vocab_opts.
 *  1. Which tokens give an id.  Exactly the tokens wakati keeps (its rules 1 and 3): EOS and dummy records never give one.
 *  2. The word is the word of the counts section's rule 2, its sharpening included: the word of a KNOWN token with an id whose word is its
 *     surface is THE DICTIONARY'S KEY OF THAT ID.  The key is the word's bytes (counts rule 3): encode and count agree on a word's identity.
 *  3. The id of a word is its index in the list, as int32 (n_words <= 2^31 - 1).  A kept token whose word is not in the list gets unk_id,
 *     which may be any int32, inside the list's range or not.  Specials such as "<pad>" are ordinary entries the caller places where they
 *     want them; an entry no token's word can equal is not an error.  The same bytes twice in the list: KGPU_ERR_INVALID_ARG, the message
 *     names both indices.  The empty word is a legal entry.
 *  4. The sequence of a sentence is [bos_id] if KGPU_VOCAB_ADD_BOS, then the ids of its kept tokens in order, then [eos_id] if
 *     KGPU_VOCAB_ADD_EOS; L(s) is its length.  A sentence with no kept token -- KGPU_SENT_INVALID_UTF8, an unreachable EOS (wakati rule 5) --
 *     still gets its bos / eos.  The status byte is what the tokenize call reports.
 *  5. Ragged output.  id_offsets (n + 1 entries, in ids, not bytes) is the exclusive scan of L; ids[id_offsets[s] + j] is element j of
 *     sentence s's sequence.  The capacity protocol is kgpu_tokenize_batch_words': on KGPU_ERR_CAPACITY *n_ids is the exact count, and
 *     nothing was written (the device form always; a host call whose input is one chunk -- up to 2 MiB and 1024 sentences -- too; a larger
 *     host call may have delivered the chunks that fitted).
 *  6. Padded output (the device form only, width >= 1).  d_ids is n x width: row s is the first `width` elements of the sequence, then
 *     pad_id.  When L(s) > width and EOS was asked for, slot width - 1 holds eos_id.  id_offsets is still the exclusive scan of the
 *     UNTRUNCATED L: the caller sees truncation and can build a mask.  A capacity below n x width is KGPU_ERR_INVALID_ARG at enqueue; the
 *     padded form never returns KGPU_ERR_CAPACITY.
 *  7. Bad records (wakati rule 6) make the sync return KGPU_ERR_INVALID_ARG.
 *  8. The handle is immutable: any number of threads may use it at once.  It keeps the words handle's tables and the dictionary alive, as a
 *     counts handle does: it may outlive both handles. */
#define KGPU_VOCAB_ADD_BOS 1u
#define KGPU_VOCAB_ADD_EOS 2u
typedef struct kgpu_vocab_opts {
    uint32_t size;     /* sizeof(kgpu_vocab_opts): fields may be appended later */
    uint32_t flags;    /* KGPU_VOCAB_ADD_BOS | KGPU_VOCAB_ADD_EOS */
    int32_t unk_id;
    int32_t bos_id;    /* read only with KGPU_VOCAB_ADD_BOS */
    int32_t eos_id;    /* read only with KGPU_VOCAB_ADD_EOS */
} kgpu_vocab_opts;
typedef struct kgpu_vocab_info {
    uint32_t size;            /* in: sizeof(kgpu_vocab_info) as the caller knows it; that many bytes are written at most */
    uint32_t reserved;
    uint64_t n_words;
    uint64_t table_slots;     /* slots of the byte-keyed table (16 bytes each): a power of two, at least 2 x n_words and at least 16 */
    uint64_t key_bytes;       /* bytes of its key arena: per word its length rounded up to 8, plus 8 */
    uint64_t rows_resolved;   /* feature rows (known and unknown morphs) whose word is in the list */
} kgpu_vocab_info;
typedef struct kgpu_vocab kgpu_vocab;
/* KGPU_ERR_INVALID_ARG: a null handle, opts or out, an opts.size smaller than the struct, unknown flags, offsets that run backwards, word
 * bytes without `words`, more than 2^31 - 1 words, the same bytes twice.  The tables are built on the host and uploaded once: 4 bytes per
 * feature row, 16 per slot, and the key arena. */
int kgpu_vocab_create(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const kgpu_vocab_opts *opts,
                      kgpu_vocab **out);
void kgpu_vocab_destroy(kgpu_vocab *v);
int kgpu_vocab_get_info(const kgpu_vocab *v, kgpu_vocab_info *info);
/* The sentences of kgpu_tokenize_batch_words, tokenized and encoded (rule 5): ids has id_capacity entries, id_offsets n + 1, status n (may
 * be NULL); *n_ids (may be NULL) is the ids written, or needed. */
int kgpu_encode_batch(kgpu_vocab *v, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, int32_t *ids, uint64_t id_capacity,
                      uint64_t *id_offsets, uint8_t *status, uint64_t *n_ids);
/* The raw block of kgpu_tokenize_text_words, split and trimmed on the device, one sequence per line; that call's protocol for the two exact
 * sizes: id_offsets / status have offsets_capacity / offsets_capacity - 1 entries, n_lines and n_ids are required. */
int kgpu_encode_text(kgpu_vocab *v, const uint8_t *text, uint64_t len, int32_t *ids, uint64_t id_capacity, uint64_t *id_offsets,
                     uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_ids);
/* Device-resident: encode records that a synced kgpu_tokenize_device batch (or anyone) left in HBM, enqueued on c's stream.  width 0: ragged
 * (rule 5; pad_id is ignored), else padded (rule 6).  d_ids: id_capacity entries, 4-byte aligned; d_id_offsets: n + 1.  kgpu_ctx_sync_lines
 * waits and reports id_offsets[n].  One render, count or encode may be pending per context, whichever kind.  A context whose dictionary is not
 * the handle's: KGPU_ERR_INVALID_ARG. */
int kgpu_encode_device(kgpu_ctx *c, const kgpu_vocab *v, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                       const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                       int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id, uint64_t *d_id_offsets);

/* ---- WordPiece ids: out-of-list words split into subword ids on the device (NOT an output of the reference: the second half of the
 * "morphological tokenizer, then WordPiece" pipeline of the BERT-Japanese family) ----
 * A WordPiece vocabulary is a kgpu_vocab made by kgpu_vocab_create_wordpiece; kgpu_encode_batch, kgpu_encode_text, kgpu_encode_device,
 * kgpu_vocab_get_info and kgpu_vocab_destroy take it as they take a plain one.  A kept token gives the PIECES of its word: zero, one or many
 * ids.  These are the rules of BERT's WordpieceTokenizer, stated on bytes.  NOT claimed: equal input_ids with a real BERT-Japanese tokenizer,
 * which segments with the real IPADIC (its NFKC is available: "text normalisation" below); what is claimed is the split below.
 *  1. Which tokens, which word.  Rules 1 and 2 of "vocabulary ids", unchanged: the tokens wakati keeps; the dictionary's key for a known token
 *     whose word is its surface.
 *  2. Characters.  A character of a word starts at byte 0 and at every byte that is not 10xxxxxx: defined for any bytes, UTF-8 or not.  A
 *     piece begins and ends only at a character start or at the word's end.
 *  3. Tables.  The INITIAL table is the whole list, verbatim: the table of a plain vocabulary (a duplicate is still the verbatim-bytes
 *     duplicate of rule 3 there).  The CONTINUATION table holds every list entry that starts with the prefix and is longer than it, with the
 *     prefix stripped, under the entry's own list index.  With prefix_len == 0 the continuation table is the initial table.
 *  4. The split of a word of len bytes.
 *     a. The empty word gives no id.
 *     b. A word of more than max_word_chars characters gives [unk_id].
 *     c. Otherwise start = 0, and while start < len: take the largest end > start (a character start, or len) such that word[start:end] is in
 *        the initial table if start == 0, in the continuation table otherwise.
 *     d. No such end: the WHOLE word gives the single id unk_id; the pieces found so far are discarded.
 *     e. Otherwise the entry's id is the next piece and start = end.
 *     So a word that is listed whole gives its one id, as from a plain vocabulary; the surface "##abc" matches a list entry "##abc" at start 0.
 *  5. Sequence, ragged form, padded form, bad records, immutability: rules 4 to 8 of "vocabulary ids" with "the ids of its kept tokens" read
 *     as "the pieces of its kept tokens, in order".  A padded row may be cut INSIDE a token's pieces: it holds the first `width` elements of
 *     the sequence, and with EOS asked for the last slot of a cut row holds eos_id.  id_offsets stays the scan of the untruncated lengths.
 *  6. Capacity.  A token may give up to max_word_chars ids: no bound by the record count holds.  The protocol is rule 5's: on
 *     KGPU_ERR_CAPACITY the count is exact and nothing was written. */
typedef struct kgpu_wordpiece_opts {
    uint32_t size;            /* sizeof(kgpu_wordpiece_opts) */
    uint32_t max_word_chars;  /* 0: 100.  1..1024 */
    uint32_t prefix_len;      /* 0..8 */
    uint8_t  prefix[8];       /* the continuation prefix; a NULL opts means "##", 100 */
} kgpu_wordpiece_opts;
typedef struct kgpu_wordpiece_info {
    uint32_t size;               /* in: sizeof(kgpu_wordpiece_info) as the caller knows it; that many bytes are written at most */
    uint32_t reserved;
    uint64_t cont_words;         /* entries of the continuation table */
    uint64_t cont_table_slots;   /* its slots (16 bytes each); with prefix_len == 0 the initial table's: the table is shared, not built twice */
    uint64_t cont_key_bytes;     /* bytes of its key arena */
    uint64_t rows_whole;         /* row-determined feature rows whose word is one listed piece ... */
    uint64_t rows_split;         /* ... is several pieces ... */
    uint64_t rows_unk;           /* ... gives unk_id (too long, or no split); the empty word's rows are in none of the three */
    uint64_t row_piece_ids;      /* ids in the pool behind the rows that split */
    uint64_t max_initial_bytes;  /* the longest entry of each table in bytes: no longer prefix of a word is probed */
    uint64_t max_cont_bytes;
} kgpu_wordpiece_info;
/* kgpu_vocab_create's arguments and errors, and wp: KGPU_ERR_INVALID_ARG for a size smaller than the struct, prefix_len > 8 or max_word_chars
 * > 1024.  Beside the plain handle's tables: 8 bytes per feature row instead of 4, the pool, and the continuation table. */
int kgpu_vocab_create_wordpiece(kgpu_words *w, const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words,
                                const kgpu_vocab_opts *opts, const kgpu_wordpiece_opts *wp, kgpu_vocab **out);
int kgpu_vocab_get_wordpiece_info(const kgpu_vocab *v, kgpu_wordpiece_info *info);   /* KGPU_ERR_INVALID_ARG on a plain vocabulary */

/* ---- text normalisation: NFC / NFKC of lines on the device (NOT an output of the reference: the first stage of every MeCab-style pipeline; half-width
 * katakana, full-width ASCII, U+3231, U+2460 and U+3000 match no IPADIC key and no vocabulary line until they have been through NFKC) ----
 * The tables are derived from Unicode kgpu_normalize_unicode_version() (tools/gen_normalize_tables.py) and are dictionary-independent: the kgpu_dict *
 * of the calls below only names the device and the context pool.  They are uploaded by a handle's first normalise call (about 200 KB, counted in
 * kgpu_dict_info.device_bytes).
 *  1. Line i of the output is line i of the input, always; text_offsets has n + 1 entries.  The empty line is the empty line.
 *  2. Boundary.  A code point c has a BOUNDARY BEFORE it, for a form with decomposition D (NFD for NFC, NFKD for NFKC), when ccc(c) == 0 and the first
 *     code point f of D(c) has ccc(f) == 0, is the second member of no primary composition pair and is no Hangul V or T jamo (U+1161-1175,
 *     U+11A8-11C2).  (Not "ccc 0 and quick-check Yes": under this rule every full-width letter starts a segment of its own, and half-width KA + the
 *     half-width voiced mark are one.)
 *  3. Segment.  A segment starts at a line's first code point and at every boundary, and ends before the next boundary or at the line's end.  The
 *     normalised line is the concatenation of the normalised segments.
 *  4. Inert.  c is inert when it has a boundary before it and the form maps it to itself.  A segment of one inert code point is copied as it is
 *     (nearly all of Japanese text).  Any other segment is decomposed (the full canonical or compatibility decomposition; Hangul syllables by
 *     arithmetic), its non-starters are put into canonical order (a stable sort by combining class), and it is composed (the 941 primary pairs of
 *     Unicode 13 and Hangul LV / LVT; a non-starter is blocked as UAX #15 says).  Unassigned code points, noncharacters and private use are inert.
 *  5. Oversize.  A segment holds its first code point and KGPU_NORMALIZE_MAX_SEGMENT more after decomposition: a starter with 64 combining marks is
 *     normalised, one with 65 is not (UAX #15's stream-safe limit is 30).  A line with a longer segment is copied unchanged and gets
 *     KGPU_SENT_NOT_NORMALIZED.
 *  6. A line that is not UTF-8 is copied unchanged with KGPU_SENT_INVALID_UTF8: a later tokenize call reports the same line.
 *  7. Capacity.  The output has up to 11 times the input's bytes (U+FDFA: 3 -> 33).  KGPU_ERR_CAPACITY: *n_bytes is the exact size needed (the
 *     kgpu_tokenize_batch_lines protocol) and nothing was written; kgpu_normalize_text reports *n_lines too, and either may be what did not fit.
 *  8. An unknown form and null arguments are KGPU_ERR_INVALID_ARG, returned before anything touches a device.  The host forms take less than 4 GiB a call.
 *  9. The device result equals kgpu_normalize_host on every line, for any bytes: both run the same segment code over the same tables.  The one
 *     difference is a single line of 4 GiB or more: kgpu_normalize_host rejects it (KGPU_ERR_INVALID_ARG), kgpu_normalize_device, which never sees
 *     the lengths on the host, copies it unchanged with KGPU_SENT_NOT_NORMALIZED (positions inside a line are 32-bit). */
#define KGPU_NORMALIZE_NFC 1
#define KGPU_NORMALIZE_NFKC 2
#define KGPU_NORMALIZE_MAX_SEGMENT 64
#define KGPU_SENT_NOT_NORMALIZED 4 /* per-line status of the normalise calls: a segment was oversize (rule 5), the line is unchanged */
const char *kgpu_normalize_unicode_version(void); /* "13.0.0" */
/* Host, no device needed: one string.  status may be NULL. */
int kgpu_normalize_host(int form, const uint8_t *in, uint64_t len, uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint8_t *status);
/* Host memory in and out, normalised on the device: n lines packed as kgpu_tokenize_batch takes them.  status may be NULL. */
int kgpu_normalize_batch(kgpu_dict *d, int form, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                         uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);
/* A raw block in host memory: split + trim on the device (kgpu_split_lines_device), then normalised; the arguments of kgpu_tokenize_text_lines. */
int kgpu_normalize_text(kgpu_dict *d, int form, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                        uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes);
/* Device-resident, enqueued on c's stream: three launches whatever the batch holds.  d_text must not overlap d_utf8 (KGPU_ERR_INVALID_ARG where the
 * call can tell: d_utf8 inside d_text's text_capacity bytes).  d_text_offsets: n + 1, d_status: n.  kgpu_ctx_sync_normalize waits and reports the byte
 * count: KGPU_ERR_CAPACITY (nothing written to d_text) when it exceeds text_capacity.  One render, count, encode or normalise may be pending per
 * context, whichever kind.  The normalised buffers are what kgpu_tokenize_device takes next. */
int kgpu_normalize_device(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                          uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status);
int kgpu_ctx_sync_normalize(kgpu_ctx *c, uint64_t *n_bytes);

/* ---- source alignment: token records of normalised text mapped back to the text the caller supplied (what highlighting, span labels, search
 * offsets and de-identification need; NOT an output of the reference) ----
 * The `_aligned` normalise calls give, beside the normalised lines, the EDIT RECORDS of every line: one per segment that changed.
 *  1. A segment ("text normalisation", rule 3) gives an edit exactly when its normalised bytes differ from its source bytes.  A copied single inert
 *     code point never gives one; a walked segment that comes out byte-identical (an already composed U+00E9, a precomposed Hangul syllable) gives
 *     none either.  One edit is one segment: edits are never merged and never split.
 *  2. A line's edits are ascending and disjoint, in the source and in the normalised line.  out_len >= 1: normalisation never deletes a character.
 *  3. Between edits the two lines are byte-identical.
 *  4. A line that is copied unchanged has no edits: KGPU_SENT_INVALID_UTF8, KGPU_SENT_NOT_NORMALIZED, and every line without a walked segment.
 *  5. edit_offsets has n + 1 entries, counted in records: the exclusive scan of the lines' edit counts.  Line i's edits are
 *     edits[edit_offsets[i] .. edit_offsets[i + 1]); their positions are relative to the line.
 *  6. Capacity.  There are two exact sizes, text bytes and edit records (at most one per input byte).  KGPU_ERR_CAPACITY: BOTH are reported and
 *     nothing was written to either buffer (the kgpu_normalize_text protocol: either may be the one that did not fit).
 *  7. The device result equals kgpu_normalize_host_aligned on every line (the same segment code: "text normalisation", rule 9).  Positions are 32-bit.
 * kgpu_source_spans_* map token records through the edits: span k belongs to token k (tok_offsets is shared), and holds kgpu_token's position,
 * byte_len, start and end in SOURCE coordinates.  Every normalised character of a changed segment maps to the WHOLE source segment.  For a token t
 * of a line with edits E, with out_end(e) = e.out_pos + e.out_len, and src_end, out_char_end, src_char_end likewise:
 *  8. Start.  e = the last edit with e.out_pos <= t.position.  None: (t.position, t.start) as they are.  t.position < out_end(e): the token starts
 *     inside the edit: (e.src_pos, e.src_char).  Otherwise (t.position - out_end(e) + src_end(e), t.start - out_char_end(e) + src_char_end(e)).
 *  9. End, for byte_len > 0: q = t.position + t.byte_len, e = the last edit with e.out_pos < q.  None: (q, t.end) as they are.  q <= out_end(e): the
 *     token ends inside the edit or at its end: (src_end(e), src_char_end(e)).  Otherwise shifted as in rule 8.
 * 10. A record with byte_len == 0 (the EOS dummy): position and start by rule 8 -- for the EOS the source line's byte length and character count --,
 *     byte_len = 0, end = start + (t.end - t.start): the EOS keeps its + 3.
 * 11. Consequences.  U+3231 -> "(株)" tokenized as three tokens gives three spans that all cover U+3231.  Span starts and span ends are each
 *     non-decreasing along a sentence.  Spans overlap only inside one edit.
 * 12. Arbitrary records.  A record's fields are only compared with edit fields and added to them (32-bit, wrapping), never used as addresses: no
 *     record, a bad one of kgpu_format_words_device's rule 6 included, causes an access outside the line's edits.  Every loop is bounded by the
 *     line's edit count. */
typedef struct kgpu_norm_edit {
    uint32_t out_pos, src_pos;     /* byte offset of the segment in the normalised / the source line        */
    uint32_t out_char, src_char;   /* char index of the segment's first code point in each                  */
    uint16_t out_len, src_len;     /* bytes (a segment is <= 65 code points on either side: <= 260 bytes)   */
    uint16_t out_chars, src_chars; /* code points                                                           */
} kgpu_norm_edit;
typedef struct kgpu_span { uint32_t position, byte_len, start, end; } kgpu_span; /* kgpu_token's four fields, in SOURCE coordinates */
/* kgpu_normalize_host with the line's edits: host only, the definition of the device results.  edits may be NULL when edit_capacity is 0. */
int kgpu_normalize_host_aligned(int form, const uint8_t *in, uint64_t len, uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint8_t *status,
                                kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *n_edits);
/* kgpu_normalize_batch / kgpu_normalize_text with the edits; edit_offsets: n + 1 (offsets_capacity) entries. */
int kgpu_normalize_batch_aligned(kgpu_dict *d, int form, const uint8_t *utf8, const uint64_t *offsets, uint64_t n,
                                 uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes,
                                 kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *edit_offsets, uint64_t *n_edits);
int kgpu_normalize_text_aligned(kgpu_dict *d, int form, const uint8_t *text, uint64_t len, uint8_t *out_text, uint64_t text_capacity,
                                uint64_t *text_offsets, uint64_t offsets_capacity, uint8_t *status, uint64_t *n_lines, uint64_t *n_bytes,
                                kgpu_norm_edit *edits, uint64_t edit_capacity, uint64_t *edit_offsets, uint64_t *n_edits);
/* kgpu_normalize_device with the edits, all in device memory: four launches whatever the batch holds.  d_edit_offsets: n + 1.
 * kgpu_ctx_sync_normalize_aligned waits and reports both sizes: KGPU_ERR_CAPACITY (nothing written to d_text or d_edits) when either exceeds its
 * capacity.  One render, count, encode, normalise or span mapping may be pending per context, whichever kind. */
int kgpu_normalize_device_aligned(kgpu_ctx *c, int form, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                                  uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status,
                                  kgpu_norm_edit *d_edits, uint64_t edit_capacity, uint64_t *d_edit_offsets);
int kgpu_ctx_sync_normalize_aligned(kgpu_ctx *c, uint64_t *n_bytes, uint64_t *n_edits);
/* The spans of n sentences' records on the host: the definition of the device results.  spans: tok_offsets[n] - tok_offsets[0] records, span k of
 * the call for record tok_offsets[0] + k. */
void kgpu_source_spans_host(const kgpu_token *tokens, const uint64_t *tok_offsets, uint64_t n, const kgpu_norm_edit *edits,
                            const uint64_t *edit_offsets, kgpu_span *spans);
/* Device-resident: the spans of records a synced kgpu_tokenize_device batch (or anyone) left in HBM, one launch on c's stream; d_spans[k] belongs
 * to d_tokens[k] (d_spans 16-byte aligned: KGPU_ERR_INVALID_ARG otherwise), and nothing is stored at or behind span_capacity.  The token count is
 * read from d_tok_offsets on the device.  It takes the context's one pending render-kind slot; kgpu_ctx_sync_lines waits for it (0 bytes). */
int kgpu_source_spans_device(kgpu_ctx *c, const kgpu_token *d_tokens, const uint64_t *d_tok_offsets, uint64_t n,
                             const kgpu_norm_edit *d_edits, const uint64_t *d_edit_offsets, kgpu_span *d_spans, uint64_t span_capacity);
/* Host arrays in, computed on the device, host arrays out: kgpu_source_spans_host's arguments. */
int kgpu_source_spans_batch(kgpu_dict *d, const kgpu_token *tokens, const uint64_t *tok_offsets, uint64_t n, const kgpu_norm_edit *edits,
                            const uint64_t *edit_offsets, kgpu_span *spans);

/* ---- ids with spans: a source span and a token index for every id (what token classification, extractive QA, highlighting and label projection
 * need beside input_ids: `return_offsets_mapping` and `word_ids()` elsewhere; NOT an output of the reference) ----
 * kgpu_encode_device_spans takes kgpu_encode_device's arguments, errors and protocol -- ragged or padded (rules 4 to 8 of "vocabulary ids", rules 5
 * and 6 of "WordPiece ids"), the context's one pending render-kind slot, kgpu_ctx_sync_lines waits and reports id_offsets[n] -- and d_ids and
 * d_id_offsets are exactly what kgpu_encode_device writes for the same input.  Element e of d_spans and of d_token_index belongs to element e of
 * d_ids, in both layouts: ragged at id_offsets[s] + j, padded at s * width + j.  For a record t of sentence s:
 *  1. Specials.  bos, eos (the eos in the last slot of a cut padded row included) and every pad slot get the span {0, 0, 0, 0} and the token index
 *     -1.  They are never mapped through edits.
 *  2. Token index.  An element that comes from record k of sentence s has the index k - tok_offsets[s]: its place among the sentence's records,
 *     dropped tokens counted, so it indexes what kgpu_tokenize_device left.
 *  3. Plain vocabulary.  The one id of a kept token carries the token's own position, byte_len, start and end.
 *  4. WordPiece, surface words.  A surface word is one whose bytes are the text's (rule 2 of "vocabulary ids": for a known token the dictionary's
 *     key; a row that falls back to the surface included).  Piece j of a split of two or more pieces covers the bytes [b_j, e_j) and the characters
 *     [cb_j, ce_j) of the word, characters as in "WordPiece ids", rule 2; when the word is t.byte_len bytes long, its span is
 *     {t.position + b_j, e_j - b_j, t.start + cb_j, t.start + ce_j}.  The pieces tile the word: b_0 = cb_0 = 0, b_(j+1) = e_j, cb_(j+1) = ce_j.
 *  5. Everything else gets the token's whole span: a word that gives one id (listed whole, or unk_id by rule 4b or 4d of "WordPiece ids"), a word
 *     that is a feature column, a surface word whose length differs from t.byte_len (a crafted record) -- every element, when several pieces come
 *     from one such word.
 *  6. Edits.  With d_edits and d_edit_offsets given (the edit records of kgpu_normalize_device_aligned for the same lines), every non-special span
 *     is replaced by the span "source alignment" gives a record with its four fields (rules 8 to 10 there): three pieces that lie in one changed
 *     segment all cover that whole source segment.  Both NULL: no mapping.  Only one of the two NULL: KGPU_ERR_INVALID_ARG.
 *  7. Capacity.  On KGPU_ERR_CAPACITY nothing was written to any of the three arrays, and the count is exact.  In the padded form no slot at or
 *     beyond n x width is ever touched.
 *  8. Arbitrary records.  As in "source alignment", rule 12: a record's fields are compared and added (32-bit, wrapping), never used as addresses;
 *     no record causes an access outside the sentence's text, its edits and the three output rows.
 * d_spans: id_capacity entries, 16-byte aligned, required; d_token_index: id_capacity entries, 4-byte aligned, may be NULL.  KGPU_ERR_INVALID_ARG
 * for a null or misaligned pointer, the unpaired edit pointers, and a context whose dictionary is not the handle's.  A WordPiece handle keeps, for
 * this call, the byte and character end of every pooled piece of its rows: 8 bytes per kgpu_wordpiece_info.row_piece_ids, uploaded at creation. */
int kgpu_encode_device_spans(kgpu_ctx *c, const kgpu_vocab *v, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n,
                             const kgpu_token *d_tokens, const uint64_t *d_tok_offsets,
                             const kgpu_norm_edit *d_edits, const uint64_t *d_edit_offsets, /* both NULL: no mapping */
                             int32_t *d_ids, uint64_t id_capacity, uint64_t width, int32_t pad_id, uint64_t *d_id_offsets,
                             kgpu_span *d_spans, int32_t *d_token_index);

/* ---- model inputs: ragged id sequences packed into padded rows [R, max_length] with token_type_ids and an attention_mask -- sentence pairs,
 * truncation, overlapping stride windows (what a BERT-family model takes: `[CLS] a [SEP]` or `[CLS] a [SEP] b [SEP]`; the truncation and template
 * processing of the `tokenizers` library; NOT an output of the reference) ----
 * The pack step takes the RAGGED output of kgpu_encode_device or kgpu_encode_device_spans -- ids, their offsets, optionally their spans and token
 * indices -- and moves it; it looks at no id.  A sample is one sequence a, or a pair a, b.  ns = 2 for a single, 3 for a pair; room = max_length - ns;
 * La, Lb are the lengths after rule 1 (Lb = 0 for a single).  Sample i's rows are row_offsets[i] .. row_offsets[i + 1] of the outputs.
 *  1. Trim.  trim_front and trim_back are 0 or 1 each: that many elements are dropped from the front and from the back of EVERY input sequence, so a
 *     vocabulary that adds bos / eos itself is packed without a second handle.  A sequence shorter than its trims has length 0.
 *  2. Layout of a row over the slices a[as .. as + al) and b[bs .. bs + bl).  Single: cls_id, the a-slice, sep_id.  Pair: cls_id, the a-slice, sep_id,
 *     the b-slice, sep_id.  The remaining slots up to max_length hold pad_id.  token_type_ids is 1 on the b-slice and on the last sep_id of a pair, 0
 *     elsewhere, the pad included.  attention_mask is 1 on everything before the pad, 0 on the pad.  Spans and token indices of slice elements are
 *     copied from the input element; every special and every pad slot gets {0, 0, 0, 0} and -1, exactly as in rule 1 of "ids with spans".
 *  3. Fits.  La + Lb <= room: one row with the whole of a and b, status KGPU_PACK_OK.
 *  4. KGPU_PACK_LONGEST_FIRST when it does not fit: one row, status KGPU_PACK_CUT, both slices start at 0.  Single: al = room.  Pair: let s1 <= s2 be
 *     the two lengths.  If s1 > room then s2 = s1, else s2 = max(s1, room - s1).  If s1 + s2 > room then s1 = room / 2 and s2 = s1 + room % 2.  They
 *     go back to the sides they came from: the side that was not longer is s1; with equal lengths a is s1.  stride is ignored; KGPU_PACK_WINDOWS
 *     together with this strategy is KGPU_ERR_INVALID_ARG.
 *  5. KGPU_PACK_ONLY_FIRST / KGPU_PACK_ONLY_SECOND when it does not fit: a (b) is cut, the other side is FIXED and kept whole.  A single under
 *     ONLY_FIRST behaves as a pair with an empty fixed side; a single under ONLY_SECOND is KGPU_ERR_INVALID_ARG at the call.  w = room - the fixed
 *     side's length.  If w < 1, or KGPU_PACK_WINDOWS is set and stride >= w, the sample gets ZERO rows and status KGPU_PACK_NO_ROOM; the batch goes
 *     on.  Otherwise the status is KGPU_PACK_CUT.  Without KGPU_PACK_WINDOWS: one row, the slice [0, w) of the cut side.  With it: window k starts at
 *     k (w - stride) and is min(w, L - start) long, L the cut side's length; the last window is the first one that reaches L.  One row per window,
 *     in order, and every window repeats the fixed side whole.  Consecutive windows share `stride` elements.
 *  6. Arguments.  max_length is ns + 1 .. 65536; stride < max_length - ns; the flags and the strategy are known ones; the trims are 0 or 1;
 *     opts.size is at least the struct's.  Anything else is KGPU_ERR_INVALID_ARG, as are a null or misaligned pointer (ids, token indices and the
 *     three int32 outputs: 4 bytes; offsets: 8; spans: 16), spans out without spans in, and token indices out without token indices in.
 *  7. Capacity.  The row outputs have row_capacity rows.  row_offsets (n + 1) and status (n) are always written.  When row_offsets[n] > row_capacity
 *     NOTHING is written to any row array and the call (the sync) returns KGPU_ERR_CAPACITY with the exact row count: the protocol of "vocabulary
 *     ids", rule 5.  No slot at or beyond row_capacity x max_length is ever touched.
 *  8. Input offsets are taken as they are (they need not start at 0, and sample i + 1 need not begin where sample i ends).  An a or b range that runs
 *     backwards or past n_ids_in makes the call (the sync) return KGPU_ERR_INVALID_ARG: it is checked where the row counts are made and never used
 *     as an address; the row arrays are unspecified then.  Element values are copied, never interpreted.
 * Both id arrays and the input spans / token indices are indexed by the same offsets: element e of spans_in / tix_in belongs to ids_a[e] (ids_b[e]),
 * all of n_ids_in entries.  off_b may point into the array off_a points into (2 n sequences encoded as one batch: off_b = off_a + n). */
#define KGPU_PACK_WINDOWS 1u        /* flags: rule 5's stride windows */
#define KGPU_PACK_LONGEST_FIRST 0u  /* strategy */
#define KGPU_PACK_ONLY_FIRST 1u
#define KGPU_PACK_ONLY_SECOND 2u
#define KGPU_PACK_OK 0              /* per-sample status (uint8) */
#define KGPU_PACK_CUT 1
#define KGPU_PACK_NO_ROOM 2
typedef struct kgpu_pack_opts {
    uint32_t size;        /* sizeof(kgpu_pack_opts): fields may be appended later */
    uint32_t flags;       /* KGPU_PACK_WINDOWS */
    uint32_t strategy;    /* KGPU_PACK_LONGEST_FIRST / ONLY_FIRST / ONLY_SECOND */
    uint32_t max_length;
    uint32_t stride;
    int32_t cls_id, sep_id, pad_id;
    uint32_t trim_front, trim_back;
} kgpu_pack_opts;
/* The rule on the host, in plain C++: no device, no dictionary; the definition of the device results (both run the same statements).  All arrays in
 * host memory; ids_b / off_b NULL: singles.  spans_in, tix_in, type_ids, mask, spans, tix may each be NULL (rule 6 pairs them).  *n_rows (may be NULL):
 * row_offsets[n], written or needed. */
int kgpu_pack_host(const kgpu_pack_opts *o, uint64_t n, const int32_t *ids_a, const uint64_t *off_a, const int32_t *ids_b, const uint64_t *off_b,
                   uint64_t n_ids_in, const kgpu_span *spans_in, const int32_t *tix_in, int32_t *input_ids, int32_t *type_ids, int32_t *mask,
                   kgpu_span *spans, int32_t *tix, uint64_t row_capacity, uint64_t *row_offsets, uint8_t *status, uint64_t *n_rows);
/* Device-resident, three launches on c's stream whatever the batch holds: the row counts (one lane per sample), their scan into d_row_offsets, the
 * rows (one wavefront per output row).  Every d_* pointer is a device pointer on the context's device.  It takes the context's one pending
 * render-kind slot; kgpu_ctx_sync_lines waits and reports row_offsets[n], written or needed (rules 7 and 8 give its errors). */
int kgpu_pack_device(kgpu_ctx *c, const kgpu_pack_opts *o, uint64_t n, const int32_t *d_ids_a, const uint64_t *d_off_a, const int32_t *d_ids_b,
                     const uint64_t *d_off_b, uint64_t n_ids_in, const kgpu_span *d_spans_in, const int32_t *d_tix_in, int32_t *d_input_ids,
                     int32_t *d_type_ids, int32_t *d_mask, kgpu_span *d_spans, int32_t *d_tix, uint64_t row_capacity, uint64_t *d_row_offsets,
                     uint8_t *d_status);

/* ---- text from ids: sequences of vocabulary ids back to the words they stand for, joined into one line per sequence (the way back from
 * kgpu_encode_*: reading a model's output, showing a window, checking input_ids by eye; `tokenizers.decoders.WordPiece(prefix, cleanup=False)` stated
 * on bytes; NOT an output of the reference) ----
 * The list is the one a vocabulary handle was made from: word k is words[word_offsets[k] .. word_offsets[k + 1]), n_words of them, verbatim bytes; the
 * empty word is a legal entry.  The prefix is the continuation prefix of "WordPiece ids" (prefix_len 0..8; 0 for a plain vocabulary).
 * Input: n sequences of int32 ids, in one of two forms.  Ragged: ids and id_offsets (n + 1 entries, counted in ids), sequence s is
 * ids[id_offsets[s] .. id_offsets[s + 1]), and width == 0.  Padded: id_offsets == NULL and width >= 1, sequence s is the whole row
 * ids[s * width .. (s + 1) * width); padding is removed by the skip list, not by a length.  Any other combination is KGPU_ERR_INVALID_ARG, returned
 * before anything touches a device; so are, in the forms whose offsets lie in host memory, offsets that run backwards.  (Offsets in device memory
 * cannot be looked at by the call: a sequence whose offsets run backwards there is the empty sequence.)
 *  1. Which elements give text.  An id in the skip list gives nothing.  An id outside [0, n_words) that is not in the skip list gives nothing and
 *     sets the sequence's status byte to KGPU_DECODE_BAD_ID -- a unk_id the caller placed outside the list ("vocabulary ids", rule 3) included;
 *     otherwise the status is KGPU_DECODE_OK.  What remains are the sequence's KEPT elements, numbered k = 0, 1, ...; the word of a kept element is
 *     list entry `id`.
 *  2. Joining.  Kept element 0 contributes its word as it is, even when it starts with the prefix.  Kept element k > 0 contributes its word without
 *     its first prefix_len bytes when prefix_len > 0 and the word starts with the prefix -- the prefix is removed ONCE ("####y" gives "##y"; a word
 *     equal to the prefix gives nothing) -- and otherwise the separator followed by its word.  The empty word at k > 0 contributes the separator
 *     alone.  With prefix_len == 0 there are no continuation words: every k > 0 gets the separator.
 *  3. Output.  Packed text with text_offsets (n + 1 entries, in bytes): line s is text[text_offsets[s] .. text_offsets[s + 1]), no terminator, as in
 *     kgpu_normalize_*.  A sequence without a kept element is the empty line.  The bytes are whatever the list holds: UTF-8 only if the list and the
 *     cut points are.
 *  4. Capacity: the protocol of kgpu_tokenize_batch_lines.  text_offsets and status are always written; when text_offsets[n] > text_capacity NOTHING
 *     is written to text and the call (the sync) returns KGPU_ERR_CAPACITY with the exact size.
 *  5. The device result equals kgpu_decode_host's on every input: text, offsets and status, byte for byte.
 * opts == NULL: one space, no skip list.  KGPU_ERR_INVALID_ARG for opts.size below the struct's, a set flag, sep_len above 8, n_skip above
 * KGPU_DECODE_MAX_SKIP, prefix_len above 8, a null pointer where one is needed, and ids that are not 4-byte aligned. */
#define KGPU_DECODE_OK 0            /* per-sequence status (uint8) */
#define KGPU_DECODE_BAD_ID 1
#define KGPU_DECODE_MAX_SKIP 8
typedef struct kgpu_decode_opts {
    uint32_t size;        /* sizeof(kgpu_decode_opts): fields may be appended later */
    uint32_t flags;       /* 0; any set bit is KGPU_ERR_INVALID_ARG */
    uint32_t sep_len;     /* 0..8 */
    uint8_t sep[8];
    uint32_t n_skip;      /* 0..KGPU_DECODE_MAX_SKIP */
    int32_t skip_ids[KGPU_DECODE_MAX_SKIP];   /* any int32, inside the list's range or not */
} kgpu_decode_opts;
/* The rule on the host, in plain C++: no device, no handle; the definition of the device results (both run the same statements).  All arrays in host
 * memory.  *n_bytes (may be NULL): text_offsets[n], written or needed. */
int kgpu_decode_host(const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, const uint8_t *prefix, uint32_t prefix_len,
                     const int32_t *ids, const uint64_t *id_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *opts,
                     uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);
/* Device-resident, three launches on c's stream whatever the batch holds: the lines' lengths and status bytes (one wavefront per sequence), their
 * scan into d_text_offsets, the bytes.  Every d_* pointer is a device pointer on the context's device (d_id_offsets NULL: padded).  A WordPiece
 * handle supplies its own prefix, a plain handle none.  It takes the context's one pending render-kind slot (one render, count, encode, normalise,
 * span mapping, pack or decode may be pending per context); kgpu_ctx_sync_lines waits and reports text_offsets[n], written or needed.  A context
 * whose dictionary is not the handle's is KGPU_ERR_INVALID_ARG.  The handle's first decode call uploads an id -> word table of 4 bytes per list
 * entry, once; a handle that never decodes never holds it, and kgpu_vocab_get_info is what it was. */
int kgpu_decode_device(kgpu_ctx *c, const kgpu_vocab *v, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, uint64_t width,
                       const kgpu_decode_opts *opts, uint8_t *d_text, uint64_t text_capacity, uint64_t *d_text_offsets, uint8_t *d_status);
/* Host memory in, host memory out, computed on the device: kgpu_decode_host's arguments behind the handle.  This is the SIMPLE route, not a
 * pipelined path: per chunk of sequences one upload, one kgpu_decode_device, one sync and one download on a context of the dictionary's pool, one
 * chunk after the other.  A call of one chunk writes nothing on KGPU_ERR_CAPACITY; with several, the chunks in front of the one that did not fit
 * have been delivered.  *n_bytes is exact either way. */
int kgpu_decode_batch(kgpu_vocab *v, const int32_t *ids, const uint64_t *id_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *opts,
                      uint8_t *text, uint64_t text_capacity, uint64_t *text_offsets, uint8_t *status, uint64_t *n_bytes);

/* ---- N-best paths: the k lowest-cost tokenizations of each sentence (NOT an output of the reference: what `mecab -N k` prints) ----
 * Take the lattice of Lattice::build (src/lattice.rs:29-114): nodes in insertion order, BOS = 0, EOS last; the predecessors of a node t are the nodes
 * ending at t.char_pos (EOS has char_pos = C, the sentence's characters).  Take n_best = k with 1 <= k <= KGPU_NBEST_MAX.
 *  The list per node.  Every node t gets a ranked list L(t) of at most k entries (cost, pred, pred_rank).
 *    L(BOS) = [(0, none, none)].
 *    For every other t the candidates are (L(j)[r].cost + t.cost + M[j.right_id][t.left_id], j, r) for every predecessor j and every rank r that L(j)
 *    has; the arithmetic is int32.  A candidate whose cost is >= 1 << 30 is dropped: the reference's clamp and its strict '<' do the same
 *    (src/lattice.rs:117,135-136).  L(t) holds the k smallest candidates under the lexicographic order of the triple (cost, j, r), sorted.
 *  The result is L(EOS), best first.  Path number r is read back through (pred, pred_rank) down to BOS; BOS is dropped and EOS is kept, as tokenize does,
 *  and each node on the path becomes the same 24-byte kgpu_token that tokenize emits for it.  The definition works on real BOS -> EOS paths only: a
 *  node that nothing reachable ends at has an empty list.
 * What follows from the rule:
 *  1. Paths compare by cost, then backwards from the end: the order on paths is cost first, then (backwards from EOS) the lower predecessor node
 *     index, then recursively the order of the two prefixes.  A brute-force enumeration of all paths sorted with that recursive comparator gives
 *     exactly the first k (tests/nbest_ref.py does that).
 *  2. Path 0 is tokenize's path: it holds exactly the records of kgpu_tokenize_batch whenever EOS is truly reachable -- the lowest-index tie-break of
 *     the strict '<' is the (cost, j) order, and an unreachable predecessor's 1 << 30 candidate can never tie with or beat a real one.
 *  3. Unreachable EOS gives 0 paths: where the reference returns [] or a chain whose head is an unreachable node (src/lattice.rs:144-153) there is no
 *     real path; the sentence gets 0 paths and status KGPU_SENT_OK.
 *  4. Fewer than k paths is not an error: a sentence with fewer than k paths gives them all.  "" gives one path, [EOS], with cost M[0][0].
 *  5. Invalid UTF-8: the sentence gets KGPU_SENT_INVALID_UTF8 and 0 paths.
 *  6. Too large: a lattice, with its lists (8 k N bytes for N nodes), that does not fit the largest scratch arena gets KGPU_SENT_NO_SCRATCH and 0 paths,
 *     as in kgpu_graphviz_batch; the same holds for a lattice of 2^26 nodes or more.
 * Output: sentence i's paths are path_offsets[i] .. path_offsets[i + 1] (n + 1 entries); path p has cost costs[p] and the records
 * tokens[tok_offsets[p] .. tok_offsets[p + 1]) (tok_offsets: one entry more than there are paths). */
#define KGPU_NBEST_MAX 64
/* The rule on the host, in plain C++ over one lattice as kgpu_lattice_dump returns it (the dictionary's own context ids): no device, no handle; the
 * definition of the device result, byte for byte.  conn: the connection matrix, element (right_id, left_id) at left_id * conn_rows + right_id
 * (connection.rs:12-14).  tok_offsets has path_capacity + 1 entries.  KGPU_ERR_CAPACITY: nothing is written but *n_paths and *n_tokens, the exact sizes
 * needed.  KGPU_ERR_INVALID_ARG: n_best 0 or above KGPU_NBEST_MAX, a null pointer where one is needed, fewer than two nodes or 2^26 of them or more,
 * and a lattice whose edges or node fields contradict each other -- an edge node out of range or not in front of the node it leads to, a node that
 * starts behind the last position, end_char < char_pos, a context id outside the matrix. */
int kgpu_nbest_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, uint32_t n_best,
                    kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs, uint64_t path_capacity,
                    uint64_t *n_paths, uint64_t *n_tokens);
/* n sentences in host memory, on the device: the general kernel leaves every lattice of a chunk (at most 256 KiB and 1024 sentences) in the scratch
 * arena, one workgroup per sentence builds the lists (a wavefront per target node), and three small launches count, scan and write the paths -- the protocol of
 * kgpu_graphviz_batch, chunk after chunk on one pooled context: a tool beside the throughput path, not a part of it.  Needs no feature tables.
 * path_offsets: n + 1 entries; tok_offsets: path_capacity + 1; n * n_best paths always suffice.  status may be NULL; n_paths and n_tokens are
 * required.  KGPU_ERR_CAPACITY: *n_paths and *n_tokens are the exact sizes needed (either may be the one that did not fit; a call whose input is one
 * chunk has written nothing but the status bytes then). */
int kgpu_tokenize_batch_nbest(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, uint32_t n_best,
                              kgpu_token *tokens, uint64_t token_capacity,
                              uint64_t *path_offsets /* n + 1 */, uint64_t *tok_offsets, int32_t *costs, uint64_t path_capacity,
                              uint8_t *status /* may be NULL */, uint64_t *n_paths, uint64_t *n_tokens);

/* ---- lattice probabilities: the lattice read as a distribution over tokenizations, P(path) proportional to exp(-theta cost(path)) -- token marginals
 * (what `mecab -m` / `mecab -a` give) and sampled paths (`mecab -l --theta`); NOT an output of the reference ----
 * Take the lattice of "N-best paths": nodes numbered by start position, BOS = 0, EOS last; the predecessors of t are the nodes ending at t.char_pos, the
 * successors of j the nodes starting at j.end_char.  Take theta, a double with 0 < theta <= KGPU_THETA_MAX = 2^64 -- the cap keeps every weight and log-sum finite: theta times a path's cost stays far below
 * the largest double, so no infinity and no NaN arises, on which a maximum would depend on its order -- (KGPU_THETA_DEFAULT = 0.75 / 800: MeCab's default theta over IPADIC's
 * cost factor).  The rule is INDEPENDENT OF ORDER by construction -- a maximum and an unsigned integer sum are -- and uses no library exp / log, so that
 * the device result is the host rule byte for byte although a bucket's slots are filled in no fixed order.
 *  Edge weight.  w(j, t) = -theta * (double)(M[j.right_id][t.left_id] + t.cost): the integer sum is exact, then one multiplication.
 *  Forward.  alpha[BOS] = 0.  For every other t, in node order: a_j = alpha[j] + w(j, t) over the predecessors j with finite alpha[j]; m = max a_j;
 *    S = sum_j fix(kexp(a_j - m)), an unsigned 64-bit integer sum; alpha[t] = m + klog(S * 2^-40).  fix(x) is x * 2^40 rounded to the nearest integer
 *    (ties to even); kexp(0) is exactly 1, so S >= 2^40.  A node with no finite predecessor has alpha = -inf.
 *  Backward.  beta[EOS] = 0.  For every other j, by descending end position, over the successors t with finite beta[t]: the same recursion with
 *    b_t = beta[t] + w(j, t).
 *  Results.  log_z = alpha[EOS].  A node's marginal is kexp(min(0, (alpha[t] + beta[t]) - log_z)).  best_logprob = -theta * (double)dp(EOS) - log_z, dp(EOS)
 *    tokenize's cost.  An unreachable EOS gives log_z = best_logprob = -inf, no records and status KGPU_SENT_OK, as N-best gives no paths; so does (with its
 *    own status) a sentence that is not UTF-8 or does not fit.
 *  kexp, klog (kanpyo_amd/csrc/kgpu_prob_core.h, compiled for host and device).  IEEE-754 double + - x, fma only where the source spells one
 *    (#pragma clang fp contract(off): the device would fuse a * b + c, the host would not), comparisons and integer operations; no libm function, no
 *    division.  kexp(x) for x <= 0: exactly 0 below -32, absolute error <= 2^-46.  klog(x) for positive normal x: error <= 2^-46 * max(1, |log x|).
 *    u64 -> double is (double)hi * 2^32 + (double)lo, one rounding.
 *  Limits.  N < 2^24 nodes, so S cannot overflow; a larger lattice, or one whose slabs (16 N + N bytes for the marginals, 8 N + 4 (C + 2) n_samples for the
 *    samples) do not fit the largest scratch arena, gets KGPU_SENT_NO_SCRATCH.  NO 2^30 clamp applies to the sums: every real BOS -> EOS path counts,
 *    which differs from N-best's cut-off only at cost extremes (a path whose prefix reaches 2^30 is no N-best path; here it has its weight).
 *  Marginals out.  KGPU_MARGINAL_BEST: the nodes tokenize's backtrace visits (the chain over the best predecessors from EOS) -- tokenize's own records, path
 *    0 of N-best wherever that equals them -- each with its marginal, EOS last with 1.  (The chain is the 2^30-clamped Viterbi state's, the sums have no clamp: at cost extremes EOS may
 *    have a finite alpha and no best predecessor.  The sentence then has NO KGPU_MARGINAL_BEST records, on_best is 0 everywhere, and best_logprob is
 *    -theta * 2^30 - log_z, dp(EOS) being the clamp; log_z and KGPU_MARGINAL_ALL are what they always are.)  KGPU_MARGINAL_ALL: every node but BOS with finite alpha and beta
 *    and marginal >= min_prob (0 <= min_prob <= 1), in node order, on_best[r] = 1 where the node is one of KGPU_MARGINAL_BEST's.  Sentence i's records are
 *    tok_offsets[i] .. tok_offsets[i + 1]; probs and on_best are parallel to tokens.
 *  Sampling.  Sample i of sentence s -- s the sentence's index IN THE CALL -- walks back from EOS: at node t it takes the predecessor j (finite alpha)
 *    that maximises (alpha[j] + w(j, t)) + G, the lower j at a tie, G = -klog(-klog(u)), u = (2 h + 1) * 2^-53 with h the top 52 bits of a hash of
 *    (seed, s, i, t, j): splitmix64's output function applied per word, hash = mix(mix(mix(mix(mix(seed) ^ s) ^ i) ^ t) ^ j).  u is exactly a double strictly
 *    inside (0, 1).  This is the Gumbel-max trick: no normalising sum, no order among the candidates.  A sampled path's cost is the int32 sum of its edge
 *    costs, accumulated in int64 and saturated.  The output has N-best's format; a sentence with a reachable EOS gives exactly n_samples paths (the same
 *    path may come more than once), 1 <= n_samples <= KGPU_SAMPLES_MAX. */
#define KGPU_MARGINAL_BEST 0u
#define KGPU_MARGINAL_ALL 1u
#define KGPU_SAMPLES_MAX 256
#define KGPU_THETA_DEFAULT (0.75 / 800.0)
#define KGPU_THETA_MAX 18446744073709551616.0 /* 2^64 */
/* The rule on the host, in plain C++ over one lattice as kgpu_lattice_dump returns it (the dictionary's own context ids; conn as for kgpu_nbest_host): no
 * device, no handle; the definition of the device results, byte for byte.  KGPU_ERR_CAPACITY: nothing is written but the sizes (and log_z, best_logprob).
 * KGPU_ERR_INVALID_ARG: a theta that is not above 0 and at most KGPU_THETA_MAX (a NaN included), an unknown select, min_prob outside [0, 1], n_samples 0 or above KGPU_SAMPLES_MAX, a null
 * pointer where one is needed, fewer than two nodes or 2^24 of them or more, and a lattice whose edges or node fields contradict each other (as
 * kgpu_nbest_host; also nodes that are not numbered by start position, a node without characters between BOS and EOS, a best predecessor that is not in
 * front of its node).  tok_offsets of the samples has path_capacity + 1 entries. */
int kgpu_marginals_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, double theta, uint32_t select,
                        double min_prob, kgpu_token *tokens, uint64_t token_capacity, double *probs, uint8_t *on_best, double *log_z,
                        double *best_logprob, uint64_t *n_tokens);
int kgpu_samples_host(const kgpu_lattice *lattice, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols, double theta, uint32_t n_samples,
                      uint64_t seed, uint64_t sentence_index, kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets, int32_t *costs,
                      uint64_t path_capacity, uint64_t *n_paths, uint64_t *n_tokens);
/* (tests) kexp / klog over n doubles on the host; the library's test-only export kgpu_debug_prob_device runs the same two functions on a device */
void kgpu_prob_exp_host(const double *x, uint64_t n, double *out);
void kgpu_prob_log_host(const double *x, uint64_t n, double *out);
/* n sentences in host memory, on the device, by kgpu_tokenize_batch_nbest's protocol (chunks of at most 256 KiB and 1024 sentences on one pooled context,
 * the general kernel leaving every lattice in the scratch arena): a forward kernel (one workgroup per sentence, a wavefront per target node), then the
 * backward kernel and count / scan / write (marginals), or one wavefront per (sentence, sample) and scan / write (samples).  Tools beside the throughput
 * path.  Need no feature tables.  tok_offsets of the marginals, log_z and best_logprob: n + 1, n and n entries; the samples' arrays as N-best's, n * n_samples
 * paths always suffice.  status may be NULL.  KGPU_ERR_CAPACITY: the sizes reported are exact; a call whose input is one chunk has written nothing but
 * the per-sentence arrays then. */
int kgpu_tokenize_batch_marginals(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, double theta, uint32_t select, double min_prob,
                                  kgpu_token *tokens, uint64_t token_capacity, double *probs, uint8_t *on_best,
                                  uint64_t *tok_offsets /* n + 1 */, double *log_z /* n */, double *best_logprob /* n */,
                                  uint8_t *status /* may be NULL */, uint64_t *n_tokens);
int kgpu_tokenize_batch_samples(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, double theta, uint32_t n_samples, uint64_t seed,
                                kgpu_token *tokens, uint64_t token_capacity,
                                uint64_t *path_offsets /* n + 1 */, uint64_t *tok_offsets, int32_t *costs, uint64_t path_capacity,
                                uint8_t *status /* may be NULL */, uint64_t *n_paths, uint64_t *n_tokens);

/* ---- search mode: one-best with a length penalty on long words, so that a compound gives way to its parts where the dictionary has them (what
 * Kuromoji, Kagome, Lindera and Sudachi offer for search indexing); extended mode also cuts unknown words into characters.  NOT an output of the
 * reference (its README lists "Support search mode" as open) ----
 * Take the lattice of "N-best paths": nodes in insertion order, BOS = 0, EOS last; the predecessors of t are the nodes ending at t.char_pos.
 *  Options.  kgpu_mode_opts: mode is KGPU_MODE_NORMAL, _SEARCH or _EXTENDED; kanji_length, kanji_penalty, other_length, other_penalty default to 2,
 *    3000, 7, 1700 (KGPU_MODE_OPTS_DEFAULT: the constants of Kuromoji and Kagome).  A non-zero reserved word or a mode above 2 is KGPU_ERR_INVALID_ARG.
 *    KGPU_MODE_NORMAL ignores the four numbers: every penalty is 0.
 *  Kanji.  A code point is kanji iff it is U+3005, U+3007, or in U+3400..4DBF, U+4E00..9FFF, U+F900..FAFF or U+20000..3FFFF.  This list IS the rule;
 *    it is not claimed to equal Unicode's Han script property.
 *  Penalty of a node t.  BOS and EOS: 0.  Known and Unknown nodes alike, with L = t.end_char - t.char_pos: if L > kanji_length and all L characters
 *    are kanji, (L - kanji_length) * kanji_penalty; otherwise, if L > other_length, (L - other_length) * other_penalty; otherwise 0.  The product is
 *    formed in 64 bits and capped at 1 << 29, so that a candidate dp[j] + cost + penalty + M cannot wrap an int32.
 *  Forward.  The reference's forward as written (src/lattice.rs:116-142) with t.cost + penalty(t) where it has t.cost: dp[t] starts at 1 << 30; a BOS
 *    predecessor counts 0; tot = min(dp[j] + t.cost + penalty(t) + M[j.right_id][t.left_id], 1 << 30) in int32; a candidate is accepted iff it is
 *    strictly less, so among equals the lowest predecessor index wins.  Stated without an order: dp[t], pre[t] are the minimum of the key (tot, j)
 *    over the candidates with tot < 1 << 30 (a bucket's slots are filled in no fixed order on the device).  The reference's quirk is KEPT: an unreachable
 *    predecessor's 1 << 30 plus a negative cost is below 1 << 30 and is accepted.  With all penalties 0 the result is tokenize's on every sentence.
 *  Backtrace.  The reference's (src/lattice.rs:144-153): from EOS along pre while there is one; the chain's head is dropped, EOS is kept.  No records
 *    where EOS has no predecessor.
 *  Records.  The 24-byte kgpu_token tokenize emits for each node.  In KGPU_MODE_EXTENDED a record of class Unknown with more than one character is
 *    replaced by one record per character c, ascending: the same id and class, start = c, end = c + 1, position and byte_len that character's.
 *    costs[i] = dp[EOS] under the penalised costs, 1 << 30 where nothing was accepted (or the sentence has status 1 or 2).
 *  Statuses.  As in the N-best call: invalid UTF-8 gives KGPU_SENT_INVALID_UTF8 and no records; a lattice that, with its slab of 8 N + 4 (C + 1)
 *    bytes, does not fit the largest scratch arena gives KGPU_SENT_NO_SCRATCH and no records. */
#define KGPU_MODE_NORMAL 0u
#define KGPU_MODE_SEARCH 1u
#define KGPU_MODE_EXTENDED 2u
typedef struct kgpu_mode_opts {
    uint32_t mode;
    uint32_t kanji_length, kanji_penalty, other_length, other_penalty;
    uint32_t reserved[3]; /* 0 */
} kgpu_mode_opts;
#define KGPU_MODE_OPTS_DEFAULT(m) {(m), 2u, 3000u, 7u, 1700u, {0u, 0u, 0u}}
/* The rule on the host, in plain C++ over one lattice as kgpu_lattice_dump returns it and the sentence's bytes: no device, no handle; the definition of
 * the device result, byte for byte.  conn as for kgpu_nbest_host.  KGPU_ERR_CAPACITY: nothing is written but *n_tokens, the exact count.
 * KGPU_ERR_INVALID_ARG: invalid options, a null pointer where one is needed, text that is not UTF-8, and a lattice that contradicts itself or the text
 * (kgpu_nbest_host's checks; also a node whose byte_pos + byte_len lies beyond len, or whose end_char lies beyond the text's characters). */
int kgpu_mode_host(const kgpu_lattice *lattice, const uint8_t *utf8, uint64_t len, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols,
                   const kgpu_mode_opts *opts, kgpu_token *tokens, uint64_t token_capacity, uint64_t *n_tokens, int32_t *cost);
/* n sentences in host memory, on the device, by kgpu_tokenize_batch_nbest's protocol (chunks of at most 256 KiB and 1024 sentences on one pooled context,
 * the general kernel leaving every lattice in the scratch arena): a forward kernel (one workgroup per sentence, a wavefront per target node), then count /
 * scan / write.  A tool beside the throughput path.  Needs no feature tables.  tok_offsets: n + 1 entries; costs (n) and status may be NULL.
 * KGPU_ERR_CAPACITY: *n_tokens is exact; a call whose input is one chunk has written nothing but the per-sentence arrays then. */
int kgpu_tokenize_batch_mode(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_mode_opts *opts,
                             kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets /* n + 1 */, int32_t *costs /* n, may be NULL */,
                             uint8_t *status /* may be NULL */, uint64_t *n_tokens);

/* ---- sentences: lines cut into sentences on the device (NOT an output of the reference: a MeCab-style tokenizer is fed sentences, and every Japanese
 * corpus pipeline cuts its paragraphs at the full stop first, keeping quoted speech together) ----
 * The input is n lines as every packed call takes them; the rule is stated on bytes and applies to each line by itself.
 *  1. Classes.  A class is found by the occurrence of a code point's complete UTF-8 encoding inside the line, as kgpu_split_lines finds White_Space,
 *     on invalid text too; occurrences cannot overlap (a lead byte is never a continuation byte).
 *     TERMINATOR: U+3002, U+FF61, U+FF01, U+FF1F, '!' and '?' ('.' and U+FF0E are none: decimals, URLs, abbreviations) -- or the up to 16 scalar values
 *     of the options, each >= U+0021, no surrogate, no White_Space and no bracket (else KGPU_ERR_INVALID_ARG).
 *     OPENER: U+300C U+300E U+FF08 '(' U+FF3B '[' U+FF5B '{' U+3008 U+300A U+3010 U+3014 U+FF62.
 *     CLOSER: U+300D U+300F U+FF09 ')' U+FF3D ']' U+FF5D '}' U+3009 U+300B U+3011 U+3015 U+FF63.  Bracket kinds are not told apart.
 *     SPACE: the 25 White_Space code points of kgpu_split_lines.
 *  2. Enclosing depth.  Brackets are matched within the line as a stack would; a closer with nothing open matches nothing, and neither does an opener
 *     that never closes in its line.  eff(j) is the number of matched pairs (o, c) with o <= j < c.  Equally, with r(j) = openers minus closers over
 *     0..j, P(j) = min(0, min r(0..j)) and S(j) = min r(j..end): eff(j) = r(j) - max(P(j), S(j)).
 *  3. Boundary.  One lies behind character i iff c_i is a terminator, c_(i+1) is none (or the line ends there: a run stays whole) and eff(i) = 0.
 *  4. Sentences.  A line's first sentence starts at byte 0.  Behind a boundary the next one starts at the first character that is not SPACE; if only
 *     SPACE follows up to the line's end there is no further sentence and those bytes stay in the last one.  Nothing else is trimmed: a line's bytes
 *     are its sentences plus the SPACE dropped between two of them, every line gives one sentence at least (the empty line an empty one), and a line
 *     without a boundary comes back as it was.
 *  5. Output.  The sentences packed back to back in line order (the input's byte count always suffices), out_offsets[S + 1], and one kgpu_sentence
 *     each: its line, where it starts in the line, and the bytes in front of it there that are not 10xxxxxx.  byte_start and char_start added to a
 *     token's position fields place the token in its line.
 *  6. Options.  NULL: the defaults.  n_terminators == 0: the default set.  KGPU_SENTENCES_NO_BRACKETS: eff is 0 everywhere.  Other flag bits and the
 *     reserved words must be 0.
 *  7. Capacity.  KGPU_ERR_CAPACITY when S exceeds sent_capacity: the exact S is reported and nothing was written (out_offsets holds
 *     sent_capacity + 1 entries).  The calls take less than 4 GiB of text.
 *  8. The device result equals kgpu_split_sentences_host byte for byte, for any bytes: both decide by kgpu_sentence_core.h.
 * Not claimed: closers directly behind a terminator run joining the sentence, a length cap, abbreviations, symmetric quotes, told-apart bracket kinds. */
#define KGPU_SENTENCES_NO_BRACKETS 1u
typedef struct kgpu_sentence {
    uint64_t line;       /* the index of the sentence's line */
    uint32_t byte_start; /* where it starts in that line */
    uint32_t char_start; /* ... and the characters in front of it there */
} kgpu_sentence;
typedef struct kgpu_sentence_opts {
    uint32_t flags;
    uint32_t n_terminators; /* 0: the default set */
    uint32_t terminators[16];
    uint32_t reserved[2]; /* 0 */
} kgpu_sentence_opts;
/* Host, no device needed.  out (offsets[n] - offsets[0] bytes suffice) and sents may be NULL where nothing can be written to them. */
int kgpu_split_sentences_host(const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_sentence_opts *opts, uint8_t *out,
                              uint64_t *out_offsets, kgpu_sentence *sents, uint64_t sent_capacity, uint64_t *n_sentences);
/* Host memory in and out, split on the device in chunks on a pooled context. */
int kgpu_split_sentences_batch(kgpu_dict *d, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_sentence_opts *opts, uint8_t *out,
                               uint64_t *out_offsets, kgpu_sentence *sents, uint64_t sent_capacity, uint64_t *n_sentences);
/* Device-resident, enqueued on c's stream: five launches whatever the batch holds (work is dealt by bytes, not by lines).  total_bytes is
 * offsets[n] - offsets[0], as kgpu_tokenize_device takes it; d_out (total_bytes) must not overlap the text; d_sents is 16-byte aligned.
 * kgpu_ctx_sync_sentences waits and reports the sentences and their bytes: KGPU_ERR_CAPACITY (nothing written) when they exceed sent_capacity.  One
 * render, count, encode, normalise or sentence split may be pending per context.  The buffers are what kgpu_tokenize_device takes next. */
int kgpu_split_sentences_device(kgpu_ctx *c, const uint8_t *d_utf8, const uint64_t *d_offsets, uint64_t n, uint64_t total_bytes,
                                const kgpu_sentence_opts *opts, uint8_t *d_out, uint64_t *d_out_offsets, kgpu_sentence *d_sents, uint64_t sent_capacity);
int kgpu_ctx_sync_sentences(kgpu_ctx *c, uint64_t *n_sentences, uint64_t *n_bytes);

/* ---- user dictionary: extra words beside the uploaded dictionary (what `mecab -u`, Kagome, Kuromoji, Lindera and Sudachi offer), matched against the
 * text and laid beside the lattice on the device; NOT an output of the reference (its README lists "support various dictionaries" as open) ----
 * Take the lattice of "N-best paths" / "search mode" for the sentence: N nodes in insertion order, BOS = 0, EOS = N - 1; the sentence has C characters.
 *  Entries.  E entries, e = 0 .. E - 1, each a key (valid UTF-8, 1 to 64 characters, at most 255 bytes), left_id and right_id (the dictionary's own
 *    context ids, inside the connection matrix) and an int16 cost.  Several entries may share a key, as MeCab CSVs do: each is its own node.  E = 0 is a
 *    valid dictionary.
 *  Matches.  Entry e matches at character position q (0 <= q < C) iff its key's bytes equal the text's bytes from that character's first byte on.  Every
 *    match is a USER NODE with start q, end q + the key's characters, and the entry's ids and cost.  User nodes are numbered N, N + 1, .. by (q, e)
 *    ascending; there are U of them.  Overlapping matches all exist.
 *  Withdrawn unknown nodes.  The reference adds unknown nodes at q only if no known word matched there or the character's category is in invoke_list
 *    (src/lattice.rs:54); an entry behaves as if it had been in the dictionary: an Unknown lattice node that starts at q is WITHDRAWN iff at least one
 *    entry matches at q, no Known lattice node starts at q, and the category of the character at q has invoke = 0.  A withdrawn node is neither a target
 *    nor a predecessor.
 *  Forward, backtrace, options.  The rule of "search mode" over the widened node set (opts NULL: KGPU_MODE_NORMAL).  A user node is penalised by its
 *    length and kanji count as any node is.  The predecessors of a target that starts at q are all nodes ending at q that are not withdrawn, lattice and
 *    user alike.  dp and pre are the minimum of the key (tot, j) over the candidates with tot < 1 << 30, j the combined index: among equal totals a
 *    lattice node wins over a user node, and a lower (q, e) over a higher.  The reference's unreachable-predecessor quirk is kept.  Nothing depends on
 *    the order in which a bucket or a table was filled.
 *  Records.  A lattice node gives the record tokenize emits for it.  A user node gives {id = e + 1, cls = KGPU_CLASS_USER, position, start, end,
 *    byte_len}.  KGPU_MODE_EXTENDED cuts Unknown nodes only.  costs[i], tok_offsets and the status bytes are kgpu_tokenize_batch_mode's.  With E = 0 the
 *    result is kgpu_tokenize_batch_mode's, byte for byte.
 *  Statuses.  Invalid UTF-8 gives KGPU_SENT_INVALID_UTF8 and no records; a lattice that, with its slab of 8 N + 32 U + 16 C + 44 bytes, does not fit the
 *    largest scratch arena, or with N + U >= 2^32 - 1, gives KGPU_SENT_NO_SCRATCH and no records.
 * Not claimed: the output of `mecab -u` (which needs MeCab and IPADIC), a cost for an entry that has none, Kuromoji's "simple" format. */
#define KGPU_CLASS_USER 3
#define KGPU_USERDICT_MAX_KEY_CHARS 64
#define KGPU_USERDICT_MAX_KEY_BYTES 255
typedef struct kgpu_userdict kgpu_userdict;
typedef struct kgpu_userdict_info {
    uint64_t entries;      /* E */
    uint64_t keys;         /* distinct keys */
    uint64_t longest_key;  /* in characters (0: E = 0) */
    uint64_t device_bytes; /* what the handle holds in device memory */
} kgpu_userdict_info;
/* A handle over d's connection matrix: entry e has the key keys[key_offsets[e] .. key_offsets[e + 1]) (E + 1 offsets from 0).  The ids are mapped once
 * to the numbering the device matrix uses.  KGPU_ERR_INVALID_ARG: an empty key, one over 64 characters or 255 bytes, one that is not UTF-8, an id
 * outside the matrix, offsets that run backwards, 2^31 entries or more.  A few kilobytes for a typical list: many handles may live over one dictionary.
 * Immutable; it holds a reference to d as a words handle does (destroy it before the dictionary; one that outlives kgpu_dict_destroy keeps the tables
 * alive until it goes). */
int kgpu_userdict_create(kgpu_dict *d, const uint8_t *keys, const uint64_t *key_offsets /* E + 1 */, const uint16_t *left_id, const uint16_t *right_id,
                         const int16_t *cost, uint64_t E, kgpu_userdict **out);
void kgpu_userdict_destroy(kgpu_userdict *u);
int kgpu_userdict_get_info(const kgpu_userdict *u, kgpu_userdict_info *info);
/* The rule on the host, in plain C++ over one lattice as kgpu_lattice_dump returns it and the sentence's bytes: no device, no handle; the definition of
 * the device result, byte for byte.  conn as for kgpu_nbest_host; invoke: one byte per character position (C of them; may be NULL when C or E is 0):
 * non-zero where the character's category is in invoke_list.  opts NULL: KGPU_MODE_NORMAL.  KGPU_ERR_CAPACITY: nothing is written but *n_tokens, the
 * exact count.  KGPU_ERR_INVALID_ARG: kgpu_mode_host's checks, kgpu_userdict_create's on the entries, lattice nodes that are not numbered by start
 * position, and a lattice with fewer positions than the text's characters + 2. */
int kgpu_userdict_host(const kgpu_lattice *lattice, const uint8_t *utf8, uint64_t len, const int16_t *conn, uint64_t conn_rows, uint64_t conn_cols,
                       const uint8_t *invoke, const uint8_t *keys, const uint64_t *key_offsets, const uint16_t *left_id, const uint16_t *right_id,
                       const int16_t *cost, uint64_t E, const kgpu_mode_opts *opts, kgpu_token *tokens, uint64_t token_capacity, uint64_t *n_tokens,
                       int32_t *cost_out);
/* n sentences in host memory, on the device, by kgpu_tokenize_batch_mode's protocol and with its error behaviour: per chunk the general kernel leaves the
 * lattices in the scratch arena; one workgroup per sentence matches the keys (a lane per start character, a hash probe per key length that exists),
 * lays the user nodes beside the lattice and runs the forward pass over both (a wavefront per target node); then count / scan / write.  A tool beside
 * the throughput path.  u must have been made over d.  opts NULL: KGPU_MODE_NORMAL. */
int kgpu_tokenize_batch_user(kgpu_dict *d, const kgpu_userdict *u, const uint8_t *utf8, const uint64_t *offsets, uint64_t n, const kgpu_mode_opts *opts,
                             kgpu_token *tokens, uint64_t token_capacity, uint64_t *tok_offsets /* n + 1 */, int32_t *costs /* n, may be NULL */,
                             uint8_t *status /* may be NULL */, uint64_t *n_tokens);

#ifdef __cplusplus
}
#endif
#endif
