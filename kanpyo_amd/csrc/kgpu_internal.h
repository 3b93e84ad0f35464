// kanpyo_amd/csrc/kgpu_internal.h -- shared between the host runtime
// (kgpu_dict.cpp, kgpu_ctx.cpp, kgpu_chain.cpp, kgpu_index_build.cpp) and the HIP kernels (kgpu_kernels.hip)
// of libkanpyo_gpu.so.  Not part of the public ABI.  Plain structs only, so it
// compiles as host C++ and as HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kanpyo_gpu.h"
#include "kgpu_normalize_core.h"
#include "kgpu_pack_core.h"
#include "kgpu_decode_core.h"
#include "kgpu_sentence_core.h"
#include "kgpu_user_core.h"

namespace kgpu {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// ---- HBM-resident dictionary (uploaded once by kgpu_dict_create) ----------
struct alignas(8) DaNode {  // trie/da.rs:13-17: one {base, check} pair = one 64-bit load
    int32_t base, check;
};
struct alignas(8) Morph8 {  // morph.rs:7-11 padded to 8 bytes
    int16_t left, right, cost;
    uint16_t dup;  // IndexTable.dup[id] (index.rs:12,47) when this record is the
                   // first of its surface, else 0; rides in the padding
};
struct alignas(16) CatInfo {  // one per category byte value
    uint32_t flags;  // bit0 invoke_list[cat], bit1 group_list[cat], bit2 unk entry present
    int32_t unk_first;   // UnkDict.char_category_to_morph_id[cat].0 (unk_dict.rs:15)
    uint32_t unk_count;  //                                        .1
    uint32_t pad;
};
enum : uint32_t { CAT_INVOKE = 1u, CAT_GROUP = 2u, CAT_HAS_UNK = 4u };
// The character-level copy of the trie (kgpu_chartrie.cpp).  A node: one 16-byte load tells a walk whether the child exists (check), where its
// children are (base) and whether a key ends on it (leaf < 0: the byte-level leaf's base, i.e. -(id | dup << 21) or -id) -- no terminator probe.
struct alignas(16) CtNode { int32_t base, check, leaf, pad; };
// ... and what a walk needs to know about the character it starts with, in one 16-byte load.
struct alignas(16) CharRec {
    int32_t base, slot;   // the root's child for this character in the char-level array: its base and its slot (0: no key starts with it)
    uint16_t code;        // the character's code in the char-level array (0xFFFF: in no key)
    uint8_t cat, pad;     // char_category_def.rs:33-38, resolved (table[cp] if in range else table[0])
    int32_t leaf;         // < 0: this character alone is a key (CtNode::leaf of the root's child)
};
struct CharTrie {         // host side, before the upload
    std::vector<CtNode> da;
    std::vector<CharRec> rec;                // [65536]
    std::vector<uint32_t> nb_cp, nb_code;    // characters >= U+FFFF that occur in keys, ascending, and their codes
    uint32_t n_codes = 0;
};
bool build_char_trie(const std::vector<DaNode> &da, const uint8_t *cat, size_t cat_len, CharTrie &out);  // false: walk the bytes
// kgpu_chartrie.cpp: every key of the double array by its id (the ids that share a key through `dup`, index.rs:46-51, included): id k is
// bytes[off[k - 1] .. off[k]); an id without a key is empty
void build_key_table(const std::vector<DaNode> &da, const std::vector<std::pair<int64_t, uint64_t>> &dup, uint64_t n_morphs, std::vector<uint8_t> &bytes,
                     std::vector<uint64_t> &off);

struct DictView {
    const DaNode *da;        uint32_t da_len;
    uint32_t leaf_dup;       // 1: a leaf's base is -(id | dup << 21), dup = IndexTable.dup[id] (1023: look it up in the morph record):
                             // the device copy of the double array is re-encoded at create time so that the walk learns a surface's
                             // record count (index.rs:46-51) from the terminator node it has to load anyway
    const DaNode *first;     // [65536] per BMP code point: {node, base[node]} after walking its UTF-8 bytes from
                             // the root, or {0, byte steps attempted before the walk failed}
    const Morph8 *morph;     uint32_t n_morph;
    const Morph8 *unk_morph; uint32_t n_unk_morph;   // == morph + n_morph: one table (record of node sid: morph[sid > 0 ? sid - 1 : n_morph - 1 - sid])
    const int16_t *conn;     uint32_t conn_rows;  // element (right,left) at left*rows+right (ids frequency-ranked, see kgpu_dict.cpp)
    uint32_t bos_right, eos_left;                  // the ranked ids of context id 0 (BOS/EOS Morph(0,0,0))
    const uint8_t *cat;      uint32_t cat_len;    // char_category_def.rs:17,33-38
    const CatInfo *cinfo;                          // 256 entries
    // Character-level double array (kgpu_chartrie.cpp; nullptr: the dictionary is walked byte by byte): one dependent load per character
    // instead of one per byte.  crec: per BMP code point; nb_cp / nb_code: the few characters >= U+FFFF that occur in keys.
    const CtNode *da2;       uint32_t da2_len; uint32_t n_nb;
    const CharRec *crec;
    const uint32_t *nb_cp;   const uint32_t *nb_code;
};

// ---- per-ctx control block in device memory (zeroed before every batch) ---
struct Control {
    unsigned int ovf_count[4];        // sentences handed from launch k to launch k+1
    unsigned int late_count[4];       // ... of which only after the trie walk had been paid for
    unsigned long long arena_cursor;  // bump allocator over the scratch arena (bytes)
    unsigned int arena_overflow;      // a slab request did not fit
    unsigned int pad0;
    unsigned long long n_tokens;      // dense token count (written by the scan kernel)
    unsigned long long work[7];       // kgpu_work, only when BatchArgs::count_work
    unsigned long long phase[10];     // count_work: shader-clock cycles per phase of the LDS kernel (the PROF instantiations of kgpu_pool.hip and kgpu_window.hip).  Otherwise: [why] counts the
                                      // sentences the windowed kernel handed on by the limit they ran into (kgpu_routing::window_handed) -- its non-PROF instantiations are the only writers then:
                                      // the pool kernel flushes its clocks under PROF alone (and into BatchArgs::stat_slots in a KGPU_STEP_TIMING build), kgpu_kernels.hip never writes the field
    unsigned int waves_done;          // single-launch small calls: wavefronts through with their sentence ...
    unsigned int waves_copied;        // ... and through with moving its tokens to the caller's (pinned) buffers
    unsigned int small_flag;          // the call's sequence number, stored LAST into the host copy: the host polls it
    unsigned int pack_overflow;       // compact records: a token did not fit kgpu_token8 (chars > 4095 or bytes > 262143): the host falls back to 24-byte records
    unsigned int window_fail;         // the windowed long-sentence kernel met a sentence it cannot hold AND had no list to hand it on to: the host reruns the batch with the HBM-lattice kernel
    unsigned int small_abort;         // ... a wavefront gave up waiting at the rendezvous: the host redoes the call on the general path
    unsigned int win_ticket;          // the windowed kernel's ordinary form: next entry of its work list (its workgroups claim sentences one by one)
    unsigned int pad3;
    unsigned long long dump[8];       // kgpu_lattice_dump: the sentence's lattice descriptor (the LAT_* words below)
};

struct BatchArgs {
    const uint8_t *utf8;          // concatenated sentences
    const uint64_t *offsets;      // n+1
    uint64_t n;
    Control *ctl;
    uint8_t *arena;  uint64_t arena_bytes;
    kgpu_token *stage;            // staging tokens: sentence s owns slots [off[s]-off[0]+s, +B_s+1)
    uint32_t *tok_count;          // n
    uint8_t *status;              // n
    kgpu_token *out;  uint64_t out_cap;      // dense output
    uint64_t *tok_offsets;        // n+1
    uint32_t count_work;          // accumulate kgpu_work into ctl->work (slow; off in timed runs)
    uint32_t *ovf[4];             // n entries each: work lists of launches 1.. (filled by the launch before)
    uint32_t est_q8;              // expected LDS bytes per input byte (x256): reservation size and length routing
    uint32_t dump_lattice;        // general kernel: leave the slab offsets of the (single) sentence in ctl->dump
    Control *fused_host;          // non-null: single-launch small call -- the pool kernel also scans, compacts into the (pinned,
    uint32_t fused_seq;           // device-mapped) output and publishes the control block with this sequence number
    unsigned long long *stat_slots;  // profiling runs: STAT_SLOTS x STAT_WORDS counters, one slot per wavefront of the pool launch
    // compact result records (host-buffer path, kgpu_tokenize_device_compact): when out8 is set the compaction kernel writes 8-byte
    // kgpu_token8 records (and per sentence the first token's position / start) instead of 24-byte kgpu_token records;
    // out8 / first8 may be device-mapped pinned host memory: the kernel's stores then ARE the device-to-host transfer
    kgpu_token8 *out8;
    uint32_t *first8;                // [2 n]: position, start of sentence s's first token (0xFFFFFFFF twice: no tokens)
    uint8_t *status8;                // optional (host path): the compaction kernel mirrors status[] there (mapped host memory)
    uint64_t *toff8;                 // optional (host path): ... and tok_offsets[] (n + 1), so that it reads its offsets from HBM, not back over PCIe
    // general kernel, whole batches (kgpu_graphviz_batch): every sentence's lattice stays in the arena behind the launch -- a fresh slab pair per sentence,
    // slab N followed by the render passes' per-node scratch (lat_scratch_*) -- and sentence s's descriptor goes to lat_desc[LAT_DESC_WORDS * s ..]
    // (the LAT_* words below).  The table is zeroed by the host.  0 everywhere else.
    uint32_t keep_lattice;
    unsigned long long *lat_desc;
};                                   // (added to by its owner, summed on the host: hot atomics on a few words would distort the run)
// The words of a kept lattice's descriptor, and of Control::dump (kgpu_lattice_dump's single sentence): k_tokenize_general writes words 0 .. 6.  LAT_OWN is the
// consumer's own word (kgpu_lattice_dev.h): the visible nodes for graphviz; the arena offset of the slab the forward kernel took for N-best, the
// probabilities and the modes.
enum : uint32_t { LAT_SLAB_A = 0, LAT_SLAB_N = 1,   // arena offsets of the sentence's two slabs
                  LAT_B = 2, LAT_C = 3, LAT_N = 4,  // its bytes, characters and nodes
                  LAT_VALID = 5,                    // 1: the lattice is there (0: invalid UTF-8 or no scratch -- the status says which; a consumer whose own slab did not fit clears it)
                  LAT_EOS_DP = 6, LAT_OWN = 7, LAT_DESC_WORDS = 8 };
// The slabs of k_tokenize_general (kgpu_kernels.hip), as kgpu_lattice_dump and the graphviz passes read them.  Slab A: u32[B + 4] arrays, in this order
// (the kernel has more behind them); slab N: nodeA uint4[N] | bucket uint4[N] | nodeB uint2[N] | pre u32[N].
enum : uint32_t { SLAB_A_CBYTE = 0, SLAB_A_USPAN = 1, SLAB_A_NB = 2, SLAB_A_BOFF = 3, SLAB_A_BFILL = 4, SLAB_A_PATH = 5 };
constexpr uint64_t SLAB_N_BYTES_PER_NODE = 44;
// keep_lattice: the graphviz passes' scratch behind slab N's arrays -- u64[N + 1] x 4 (sorted end|node, sort keys, node-line offsets, edge-group
// offsets), then u32[N] x 3 (visible id, node of a visible id, flags)
constexpr uint64_t lat_scratch_off(uint64_t N) { return (N * SLAB_N_BYTES_PER_NODE + 15) & ~15ull; }
constexpr uint64_t lat_scratch_bytes(uint64_t N) { return (N + 1) * 8 * 4 + N * 4 * 3; }
constexpr uint32_t STAT_SLOTS = 16384, STAT_WORDS = 32;  // words 0..6: Control::work, 16..25: Control::phase

// Launchers (kgpu_kernels.hip, kgpu_pool.hip, kgpu_window.hip).  `stream` is a hipStream_t.
struct Step;  // kgpu_chain.h
int launch_step(const DictView &d, const BatchArgs &a, const Step &s, uint32_t stop_after /* kgpu_ctx_set_ablation; 0 = run everything */, void *stream);
int launch_general_only(const DictView &d, const BatchArgs &a, void *stream);  // kgpu_lattice_dump: HBM-scratch kernel alone
int launch_general_keep(const DictView &d, const BatchArgs &a, void *stream);  // kgpu_graphviz_batch: ... over a whole batch, a.keep_lattice set
int launch_small_call(const DictView &d, const BatchArgs &a, void *stream);  // pool kernel alone, one sentence per wavefront
int launch_scan_compact(const BatchArgs &a, Control *host_ctl, void *stream, bool small_workgroups, bool one_launch, int mode, int *form);  // host_ctl: device pointer of the pinned result block; one_launch: Chain::aux_one_launch; mode: KGPU_AUX_LAUNCH
// What every consumer of a batch's 24-byte records reads (kgpu_records_dev.h: the lines, the wakati lines, the vocabulary ids, the word counts).
constexpr uint32_t feature_row(bool known, uint32_t n_morph, uint32_t id) { return (known ? 0u : n_morph) + id - 1; }   // known id k at row k - 1, unknown id u at n_morph + u - 1
struct RecordsBatch {
    const uint8_t *utf8;           // the batch's text, biased like BatchArgs::utf8: sentence s is utf8[offsets[s] .. offsets[s + 1])
    const uint64_t *offsets;       // n + 1
    uint64_t n;
    const kgpu_token *tokens;      // sentence s's records: tokens[tok_offsets[s] .. tok_offsets[s + 1])
    const uint64_t *tok_offsets;   // n + 1
    uint32_t n_morph, n_rows;      // feature rows = known + unknown morphs (feature_row)
    uint64_t *sent_len;            // device scratch, n + 1: each sentence's rendered units (bytes, ids), then (k_lines_scan, in place) their offsets
    uint64_t *text_offsets;        // n + 1: the scan's mirror for the caller (may be mapped host memory: the write pass reads sent_len)
    const uint8_t *status_in;      // optional: mirrored into status_out (mapped host memory) by the first pass
    uint8_t *status_out;
    unsigned long long *host_ctl;  // device pointer of pinned, mapped words: [0] total units, [1] a record out of range (the count: HostReport, kgpu_count.hip)
};
void launch_lines_scan(const RecordsBatch &b, void *stream);   // k_lines_scan alone (kgpu_format.hip): every render's second launch
// The CLI's output lines of a batch (kgpu_format.hip; reference src/bin/kanpyo.rs:174-197): `surface \t f1,f2,... \n` per token.
struct LinesArgs {
    RecordsBatch b;
    const uint8_t *feat;           // the dictionary's joined feature strings (kgpu_features.cpp) ...
    const uint32_t *feat_off;      // ... row r is feat[feat_off[r] .. feat_off[r + 1])
    uint8_t *text; uint64_t text_cap;
};
int launch_format_lines(const LinesArgs &a, void *stream);
// A words handle's table.  One entry per feature row (feature_row): where the row's word lies and whether its tokens are kept.
struct WordRow { uint32_t off, len_flags; };                 // names[off .. off + len); len_flags = len | WORD_SURFACE | WORD_DROPPED
constexpr uint32_t WORD_SURFACE = 1u << 30, WORD_DROPPED = 1u << 31, WORD_LEN_MASK = WORD_SURFACE - 1;
struct WordTable {
    const WordRow *rows;           // n_rows entries
    const uint8_t *names;          // the pool of distinct names the entries point into
    uint32_t sep;                  // the separator byte
    uint32_t drop_rowless;         // KGPU_WORDS_KEEP: a token without a row (id 0) is dropped
};
// The wakati lines of a batch (kgpu_words.hip): per sentence the words of its kept tokens joined by `sep`, then '\n'.
struct WordsArgs {
    RecordsBatch b;
    WordTable w;
    uint8_t *text; uint64_t text_cap;
};
int launch_format_words(const WordsArgs &a, void *stream);
// The word counts of a batch (kgpu_count.hip; include/kanpyo_gpu.h, "word counts"): every kept token adds one to its word's counter in a counts handle.
// A word is row-determined when the token is a known one with a row, or when its word is a pool name: those go to `dense`, one counter per feature row
// (the host resolves a row to its bytes at read-out).  Every other word -- an unknown-class surface, the surface of a token without a row -- goes to the
// byte-keyed table: open addressing over `slots`, the key's bytes copied into `arena`.
struct alignas(16) CountSlot { unsigned long long tag, count; };   // tag: 0 = free, else hash << 32 | (arena entry's offset / 8 + 1)
// An arena entry, 8-byte aligned: u32 length, u32 hash, the key's bytes.  Written whole BEFORE the slot that names it is claimed, never changed after.
constexpr uint32_t COUNT_ENTRY_HEAD = 8;
constexpr uint32_t COUNT_PARTIAL_WORDS = 4;   // per workgroup of the count launch: tokens counted, tokens that found no room, a bad record, slots claimed
constexpr uint32_t COUNT_STAT_WORDS = 8;      // the handle's device words: [0] arena cursor (bytes; may run past the capacity), [1] slots used, [2] tokens counted, [3] overflow tokens
struct CountsArgs {
    RecordsBatch b;                  // sent_len: the launch's per-workgroup totals, COUNT_PARTIAL_WORDS per workgroup (count_blocks), summed by the publishing kernel;
                                     // host_ctl: [0] tokens this launch counted, [1] bit 0: a record out of range, bit 1: a token found no room; text_offsets unused
    WordTable w;
    unsigned long long *dense;       // b.n_rows counters
    CountSlot *slots; uint32_t slot_mask;   // a power of two of slots
    uint8_t *arena; uint64_t arena_bytes;
    unsigned long long *stats;       // COUNT_STAT_WORDS
};
uint32_t count_blocks(uint64_t n);   // workgroups of the count launch
int launch_count_words(const CountsArgs &a, void *stream);
// The vocabulary ids of a batch (kgpu_encode.hip; include/kanpyo_gpu.h, "vocabulary ids"): every kept token gives one int32, the index of its word in a
// vocabulary handle's list.  A row-determined word (the count kernel's predicate) is one load from `row_id`; every other word is looked up in a frozen
// byte-keyed table of the counts table's layout (slots of {tag, id}, arena entries of {length, hash, bytes}).
struct alignas(16) VocabSlot { unsigned long long tag; int32_t id; uint32_t pad[2]; };   // tag: 0 = free, else hash << 32 | (arena entry's offset / 8 + 1)
constexpr uint32_t VOCAB_BOS = 1u, VOCAB_EOS = 2u;   // KGPU_VOCAB_ADD_BOS / _EOS
struct EncodeArgs {
    RecordsBatch b;                  // the units are ids; text_offsets: the caller's id_offsets
    WordTable w;
    const int32_t *row_id;           // b.n_rows entries: the id of the row's word (unk_id when it is not listed)
    const VocabSlot *slots; uint32_t slot_mask;   // a power of two of slots, load <= 0.5
    const uint8_t *arena;
    int32_t unk_id, bos_id, eos_id, pad_id;
    uint32_t flags;                  // VOCAB_BOS | VOCAB_EOS
    int32_t *ids; uint64_t id_cap;
    uint64_t width;                  // 0: ragged; else the padded form's row length
};
int launch_encode(const EncodeArgs &a, void *stream);
// ... with a source span and a token index per id (include/kanpyo_gpu.h, "ids with spans"): the SPANS instantiation of the write kernel.  Element e of
// spans / token_index belongs to element e of ids, in both layouts; every store is bounded as the id's store is.
struct SpanOut {
    kgpu_span *spans;                // id_cap entries, 16-byte aligned
    int32_t *token_index;            // id_cap entries, or null
    const kgpu_norm_edit *edits;     // null: the spans stay in the coordinates of the records; else line s's edits are edits[edit_offsets[s] .. edit_offsets[s + 1])
    const uint64_t *edit_offsets;    // n + 1
};
struct EncodeSpanArgs : EncodeArgs { SpanOut o; };
int launch_encode_spans(const EncodeSpanArgs &a, void *stream);
// kgpu_vocab_table.cpp (HIP-free, compiles alone): a vocabulary handle's two tables from the word table's rows, the dictionary's id -> key table and the list.
struct VocabTables {
    std::vector<int32_t> row_id;
    std::vector<VocabSlot> slots;
    std::vector<uint8_t> arena;
    uint64_t rows_resolved = 0;      // feature rows whose word is in the list
};
uint32_t vocab_key_hash(const uint8_t *p, uint64_t len);   // key_hash of kgpu_records_dev.h, restated for the host
// -> the id of these bytes in the table, or `unk`
int32_t vocab_find(const VocabTables &t, const uint8_t *p, uint64_t len, int32_t unk);
// KGPU_OK, or KGPU_ERR_INVALID_ARG with `err` saying why (the same bytes twice in the list: both indices).  key_bytes / key_off: build_key_table's (may be
// null when no known row's word is its surface).
int build_vocab_table(const WordRow *rows, size_t n_rows, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off,
                      const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, int32_t unk_id, VocabTables &out, std::string &err);
// The insert loop of both byte-keyed tables of a handle: n keys (key i is p[i], len[i] bytes, listed under id[i]) into `out.slots` / `out.arena`, which are sized
// here (slots: a power of two, at least 2 n and at least 16).  *max_len (may be null): the longest key in bytes.  The same bytes twice: KGPU_ERR_INVALID_ARG.
struct VocabKey { const uint8_t *p; uint64_t len; int32_t id; };
int fill_vocab_table(const std::vector<VocabKey> &keys, VocabTables &out, uint32_t *max_len, std::string &err);
// The bytes feature row r is resolved to, as build_vocab_table resolves it (pool name, or the dictionary's key of a known surface row); false: an unknown
// row whose word is the surface -- not row-determined.
bool vocab_row_bytes(const WordRow *rows, size_t r, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off, const uint8_t *&p, uint64_t &len);
// WordPiece ids (kgpu_wordpiece.hip; include/kanpyo_gpu.h, "WordPiece ids"): a kept token gives the greedy longest-match pieces of its word over two frozen
// byte-keyed tables -- the initial table (the whole list) for the piece at byte 0, the continuation table (the entries behind the prefix) for the rest.
struct WordpieceRow { uint32_t first, count; };   // a row-determined word's pieces: count 1: the id itself in `first`; else piece_ids[first .. first + count)
struct ByteTable { const VocabSlot *slots; uint32_t slot_mask; const uint8_t *arena; uint32_t max_bytes; };   // max_bytes: the longest entry: no longer prefix is probed
struct WordpieceArgs {
    RecordsBatch b;                  // the units are ids; text_offsets: the caller's id_offsets
    WordTable w;
    const WordpieceRow *rows;        // b.n_rows entries
    const int32_t *piece_ids;        // the pool behind the rows that split
    ByteTable initial, cont;         // (prefix_len 0: the same table twice)
    uint32_t max_chars;              // a word of more characters gives unk_id
    int32_t unk_id, bos_id, eos_id, pad_id;
    uint32_t flags;                  // VOCAB_BOS | VOCAB_EOS
    int32_t *ids; uint64_t id_cap;
    uint64_t width;                  // 0: ragged; else the padded form's row length
};
int launch_wordpiece(const WordpieceArgs &a, void *stream);
// ... with spans (SpanOut above).  piece_ends is parallel to piece_ids: the byte end and the character end of pooled piece k inside its row's word, filled for
// the rows whose word is the surface (the dictionary's key) and zero for a feature column's, which never need them.
struct PieceEnd { uint32_t byte_end, char_end; };
struct WordpieceSpanArgs : WordpieceArgs { SpanOut o; const PieceEnd *piece_ends; };
int launch_wordpiece_spans(const WordpieceSpanArgs &a, void *stream);
// kgpu_wordpiece_table.cpp (HIP-free; compiles with kgpu_vocab_table.cpp alone): the tables of a WordPiece handle.
constexpr uint32_t WORDPIECE_MAX_CHARS = 1024, WORDPIECE_DEFAULT_CHARS = 100, WORDPIECE_MAX_PREFIX = 8;
struct WordpieceTables {
    VocabTables initial;             // build_vocab_table's, verbatim: slots, arena, row_id (read by nobody on the device), rows_resolved
    VocabTables cont;                // slots and arena of the continuation entries; EMPTY when `shared`
    bool shared = false;             // prefix_len == 0: the continuation table IS the initial table
    uint32_t initial_max = 0, cont_max = 0;   // the longest entry of each table in bytes
    std::vector<WordpieceRow> rows;
    std::vector<int32_t> piece_ids;
    std::vector<PieceEnd> piece_ends;   // parallel to piece_ids (WordpieceSpanArgs)
    uint64_t cont_words = 0, rows_whole = 0, rows_split = 0, rows_unk = 0;
    const VocabTables &continuation() const { return shared ? initial : cont; }
    uint32_t continuation_max() const { return shared ? initial_max : cont_max; }
};
enum WordpieceOutcome { WP_EMPTY = 0, WP_WHOLE = 1, WP_SPLIT = 2, WP_UNK = 3 };
// The split of include/kanpyo_gpu.h, "WordPiece ids", on the host: the pieces of the len bytes at p are APPENDED to out -- and to ends (may be null), per
// piece, where it ends in the word in bytes and in characters; the one id of a word that gives unk_id ends where the word ends.
WordpieceOutcome wordpiece_split(const WordpieceTables &t, const uint8_t *p, uint64_t len, uint32_t max_chars, int32_t unk_id, std::vector<int32_t> &out,
                                 std::vector<PieceEnd> *ends = nullptr);
int build_wordpiece_tables(const WordRow *rows, size_t n_rows, size_t n_known, const uint8_t *names, const uint8_t *key_bytes, const uint64_t *key_off,
                           const uint8_t *words, const uint64_t *word_offsets, uint64_t n_words, int32_t unk_id, const uint8_t *prefix, uint32_t prefix_len,
                           uint32_t max_chars, WordpieceTables &out, std::string &err);
// The DOT documents of a batch's kept lattices (kgpu_graphviz.hip; reference src/graphviz.rs:30-163).
struct GraphvizArgs {
    const uint8_t *utf8;           // as BatchArgs::utf8 / offsets of the launch that kept the lattices
    const uint64_t *offsets;       // n + 1
    uint64_t n;
    uint8_t *arena;                // the arena the descriptors' offsets are relative to
    unsigned long long *desc;      // BatchArgs::lat_desc; the prepare pass stores a sentence's visible node count in LAT_OWN
    const int16_t *conn; uint32_t conn_rows;   // DictView::conn: the ids in the slabs index it as they are
    const uint8_t *label;          // the label pool (kgpu_features.cpp): row r is label[label_off[r] .. label_off[r + 1]), rows as LinesArgs::feat (feature_row)
    const uint32_t *label_off;
    uint32_t n_morph;
    uint32_t full_state;
    uint64_t dpi;
    uint64_t *sent_len;            // device scratch, n + 1: each document's bytes, then (k_gv_scan, in place) their offsets; [n] = the total
    uint8_t *text; uint64_t text_cap;   // the write pass: nothing is stored when sent_len[n] > text_cap
};
int launch_graphviz_measure(const GraphvizArgs &a, void *stream);   // prepare, lengths, scan: sent_len is final behind it
int launch_graphviz_write(const GraphvizArgs &a, void *stream);
// The N-best paths of a batch's kept lattices (kgpu_nbest.hip; include/kanpyo_gpu.h, "N-best paths").
struct NbestArgs {
    uint64_t n;                    // the sentences of the launch that kept the lattices
    uint32_t k;                   // n_best, 1 .. KGPU_NBEST_MAX
    Control *ctl;                  // the launch's control block: the forward kernel takes its list slabs behind the lattices' (arena_cursor, arena_overflow)
    uint8_t *arena; uint64_t arena_bytes;   // as BatchArgs::arena / arena_bytes of that launch
    unsigned long long *desc;      // BatchArgs::lat_desc; the forward kernel stores the arena offset of a sentence's lists -- u64[N][k] -- in LAT_OWN, and
                                   // clears LAT_VALID where they did not fit
    const int16_t *conn; uint32_t conn_rows;   // DictView::conn: the ids in the slabs index it as they are
    uint8_t *status;               // BatchArgs::status: KGPU_SENT_NO_SCRATCH where the lists did not fit
    uint64_t *path_len;            // device scratch, n * k + 1: the records of path (s, r) at [s * k + r] (0: no such path), then (the scan, in place) their offsets; [n * k] = the total
    uint64_t *path_offsets;        // n + 1: each sentence's paths, then (the scan, in place) their offsets; [n] = the total
    kgpu_token *tokens; uint64_t token_cap;      // the write pass: nothing is stored when path_len[n * k] > token_cap or path_offsets[n] > path_cap
    uint64_t *tok_offsets; int32_t *costs; uint64_t path_cap;   // tok_offsets: path_cap + 1
};
int launch_nbest_measure(const NbestArgs &a, void *stream);   // forward, count, scan: path_len and path_offsets are final behind it
int launch_nbest_write(const NbestArgs &a, void *stream);
// The lattice probabilities of a batch's kept lattices (kgpu_prob.hip; include/kanpyo_gpu.h, "lattice probabilities"): token marginals, or sampled paths.
struct ProbArgs {
    uint64_t n;                    // the sentences of the launch that kept the lattices
    uint64_t sent_base;            // the call's index of the launch's first sentence: a sample's hash takes the sentence's index IN THE CALL
    double theta, min_prob;
    uint32_t select;               // KGPU_MARGINAL_BEST / KGPU_MARGINAL_ALL
    uint32_t n_samples;            // 0: marginals; else 1 .. KGPU_SAMPLES_MAX
    uint64_t seed;
    Control *ctl;                  // the launch's control block: the forward kernel takes its slabs behind the lattices' (arena_cursor, arena_overflow)
    uint8_t *arena; uint64_t arena_bytes;   // as BatchArgs::arena / arena_bytes of that launch
    unsigned long long *desc;      // BatchArgs::lat_desc; the forward kernel stores the arena offset of a sentence's slab in LAT_OWN and clears LAT_VALID where
                                   // it did not fit.  The slab: alpha f64[N], then beta f64[N] | best-path bytes u8[N] (marginals) or the sampled nodes u32[n_samples][C + 2]
    const int16_t *conn; uint32_t conn_rows;   // DictView::conn: the ids in the slabs index it as they are
    uint8_t *status;               // BatchArgs::status: KGPU_SENT_NO_SCRATCH where the slab did not fit
    // marginals
    uint64_t *sent_len;            // device scratch, n + 1: each sentence's records, then (the scan, in place) their offsets = the call's tok_offsets; [n] = the total
    double *log_z, *best_logprob;  // n each
    kgpu_token *tokens; uint64_t token_cap;   // the write passes: nothing is stored when the total exceeds token_cap (samples: or the paths path_cap)
    double *probs; uint8_t *on_best;
    // samples
    uint64_t *path_len;            // device scratch, n * n_samples + 1: the records of sample (s, r), then (the scan, in place) their offsets
    uint64_t *path_offsets;        // n + 1: each sentence's paths (n_samples or 0), then their offsets
    int32_t *path_cost;            // device scratch, n * n_samples
    uint64_t *tok_offsets; int32_t *costs; uint64_t path_cap;   // tok_offsets: path_cap + 1
};
int launch_prob_marginals_measure(const ProbArgs &a, void *stream);   // forward, backward, count, scan: sent_len, log_z and best_logprob are final behind it
int launch_prob_marginals_write(const ProbArgs &a, void *stream);
int launch_prob_samples_measure(const ProbArgs &a, void *stream);     // forward, sample, scan: path_len and path_offsets are final behind it
int launch_prob_samples_write(const ProbArgs &a, void *stream);
// The search / extended mode decode of a batch's kept lattices (kgpu_mode.hip; include/kanpyo_gpu.h, "search mode").
struct ModeArgs {
    uint64_t n;                    // the sentences of the launch that kept the lattices
    kgpu_mode_opts opts;           // checked by the caller (mode_opts_valid)
    Control *ctl;                  // the launch's control block: the forward kernel takes its slabs behind the lattices' (arena_cursor, arena_overflow)
    uint8_t *arena; uint64_t arena_bytes;   // as BatchArgs::arena / arena_bytes of that launch
    const uint8_t *utf8; const uint64_t *offsets;   // BatchArgs::utf8 / offsets of that launch: the characters the penalties look at
    unsigned long long *desc;      // BatchArgs::lat_desc; the forward kernel stores the arena offset of a sentence's slab in LAT_OWN and clears LAT_VALID where
                                   // it did not fit.  The slab: state u64[N] (dp << 32 | pre), then the kanji counts u32[C + 1]
    const int16_t *conn; uint32_t conn_rows;   // DictView::conn: the ids in the slabs index it as they are
    uint8_t *status;               // BatchArgs::status: KGPU_SENT_NO_SCRATCH where the slab did not fit
    uint64_t *sent_len;            // device scratch, n + 1: each sentence's records, then (the scan, in place) their offsets = the call's tok_offsets; [n] = the total
    int32_t *costs;                // n: dp of EOS under the penalised costs (1 << 30 where nothing was accepted or the sentence has no lattice)
    kgpu_token *tokens; uint64_t token_cap;   // the write pass: nothing is stored when sent_len[n] > token_cap
};
int launch_mode_measure(const ModeArgs &a, void *stream);   // forward, count, scan: sent_len and costs are final behind it
int launch_mode_write(const ModeArgs &a, void *stream);
// The user dictionary over a batch's kept lattices (kgpu_user.hip; include/kanpyo_gpu.h, "user dictionary"): ModeArgs with the table and what tells a
// character's category.  The slab a sentence's forward workgroup takes (its arena offset in LAT_OWN): a 16-byte head {U}, the user nodes uint4[U], the
// state u64[N + U], then u32 arrays -- kanji counts [C + 1], user nodes by start [C + 2], by end [C + 2] twice (offsets, fill cursors), the end-sorted
// user nodes [U], their entries [U].
struct UserArgs {
    ModeArgs m;
    UserTableView t;               // in device memory
    const uint8_t *cat; uint32_t cat_len; const CatInfo *cinfo;   // DictView's
};
int launch_user_measure(const UserArgs &a, void *stream);   // forward (match, lay out, sweep), count, scan: sent_len and costs are final behind it
int launch_user_write(const UserArgs &a, void *stream);
// kgpu_user_table.cpp (HIP-free, compiles alone): a user dictionary's table in host memory.  left_rank / right_rank (null or empty: identity): the
// numbering of the matrix the table is used with, by the dictionary's own id.
struct UserTable {
    std::vector<uint64_t> slots; std::vector<UserGroup> groups; std::vector<UserEntry> ents; std::vector<uint8_t> arena;
    uint64_t len_mask = 0; uint32_t longest = 0;
    UserTableView view() const;
};
int build_user_table(const char *who, const uint8_t *keys, const uint64_t *key_offsets, const uint16_t *left_id, const uint16_t *right_id, const int16_t *cost,
                     uint64_t E, uint64_t conn_rows, uint64_t conn_cols, const std::vector<uint32_t> *left_rank, const std::vector<uint32_t> *right_rank,
                     UserTable &out);
int launch_prob_eval(const double *d_x, uint64_t n, double *d_out, uint32_t which, void *stream);   // (tests) kexp / klog over an array
// read_line + trim_end over a block in HBM (kgpu_split.hip; reference src/bin/kanpyo.rs:114-122).
struct SplitTile { uint32_t x, y, z, w; };   // one tile's aggregate, then its carry (kgpu_split.hip says which word is what)
struct SplitArgs {
    const uint8_t *in; uint64_t len;   // the block (any alignment), len < 2^32
    uint8_t *out;                      // the trimmed lines packed back to back: len bytes always suffice
    uint64_t *offsets; uint64_t off_cap;   // lines + 1 entries; nothing is stored when they do not fit
    SplitTile *agg; uint32_t ntiles;   // device scratch, ntiles + 1 entries (split_tiles)
    unsigned long long *host_ctl;      // device pointer of pinned, mapped words: [0] lines, [1] packed bytes
};
uint32_t split_tiles(const uint8_t *d_in, uint64_t len);
int launch_split_lines(const SplitArgs &a, void *stream);
// Lines cut into sentences (kgpu_sentence.hip; include/kanpyo_gpu.h, "sentences").  The per-tile scratch: what the two reduce launches leave and what the
// two carry launches make of it (kgpu_sentence.hip says which word is what); carry_b[ntiles] holds the totals.
struct SentAggA { int32_t fb, fa, bb, ba; uint32_t fixed, pad; };
struct SentCarryA { int32_t v_in, u_in; };
struct SentAggB { uint64_t lines; uint32_t ns, dropped, head, tail, kinds, nc; };
struct SentCarryB { uint64_t sent_before; uint32_t kept_before, char_in, fl, pad; };
struct SentArgs {
    const uint8_t *utf8; const uint64_t *offsets; uint64_t n;   // line i is utf8[offsets[i] .. offsets[i + 1])
    uint64_t total;                    // offsets[n] - offsets[0] as the caller states it, < 2^32: no byte behind it is read
    SentRule rule;                     // kgpu_sentence_core.h: the terminators, and whether brackets count
    uint8_t *out;                      // the sentences packed back to back: total bytes always suffice
    uint64_t *out_offsets; kgpu_sentence *sents; uint64_t sent_cap;   // sent_cap + 1 offsets, sent_cap records; nothing is stored when S > sent_cap
    SentAggA *agg_a; SentCarryA *carry_a; SentAggB *agg_b; SentCarryB *carry_b; uint64_t *tile_lines; uint32_t ntiles;   // device scratch (sent_scratch_bytes)
    unsigned long long *host_ctl;      // device pointer of pinned, mapped words: [0] sentences, [1] packed bytes
};
uint32_t sent_tiles(uint64_t total);
inline size_t sent_scratch_bytes(uint32_t ntiles) { return ((size_t)ntiles + 1) * (sizeof(SentAggA) + sizeof(SentCarryA) + sizeof(SentAggB) + sizeof(SentCarryB) + 16); }
void sent_place_scratch(SentArgs &a, void *scratch);   // a.ntiles set: the four arrays inside a block of sent_scratch_bytes (8-byte aligned)
int launch_split_sentences(const SentArgs &a, void *stream);
// kgpu_sentence_host.cpp (HIP-free, compiles alone): the options checked and turned into the rule -> KGPU_OK, or KGPU_ERR_INVALID_ARG with the error set
int sent_rule_from_opts(const char *who, const kgpu_sentence_opts *opts, SentRule &rule);

// Text normalisation (kgpu_normalize.hip; include/kanpyo_gpu.h, "text normalisation"): line i of the batch, NFC or NFKC, into text[text_offsets[i] ..).
struct NormArgs {
    NormTables t;                      // the tables in device memory (kgpu_normalize_core.h)
    uint32_t form;                     // NORM_FORM_NFC / NORM_FORM_NFKC
    const uint8_t *utf8;               // line i is utf8[offsets[i] .. offsets[i + 1])
    const uint64_t *offsets;           // n + 1
    uint64_t n;
    uint64_t *sent_len;                // device scratch, n + 1: each line's output bytes, then (k_lines_scan, in place) their offsets
    uint8_t *mode;                     // device scratch, n: how the write pass treats the line
    uint64_t *text_offsets;            // n + 1: the scan's mirror for the caller
    uint8_t *status;                   // n
    uint8_t *text; uint64_t text_cap;  // nothing is stored when sent_len[n] > text_cap
    unsigned long long *host_ctl;      // device pointer of pinned, mapped words: [0] the output's bytes
};
int launch_normalize(const NormArgs &a, void *stream);
// ... with the lines' edit records (include/kanpyo_gpu.h, "source alignment"): the ALIGN instantiations of the same two kernels and a second scan
struct NormAlignArgs : NormArgs {
    uint64_t *edit_len;                // device scratch, n + 1: each line's edits, then (k_lines_scan, in place) their offsets
    uint64_t *edit_offsets;            // n + 1: that scan's mirror for the caller
    kgpu_norm_edit *edits; uint64_t edit_cap;   // nothing is stored, text included, when sent_len[n] > text_cap or edit_len[n] > edit_cap
};                                     // host_ctl: [1] the edits
int launch_normalize_aligned(const NormAlignArgs &a, void *stream);
// The source spans of a batch's records (kgpu_align.hip): spans[k] = tokens[k] mapped through its line's edits.  b: tokens, tok_offsets and n; offsets is
// any array of n + 1 readable words (the text is not looked at).
struct SpansArgs {
    RecordsBatch b;
    const kgpu_norm_edit *edits;       // line s's edits: edits[edit_offsets[s] .. edit_offsets[s + 1])
    const uint64_t *edit_offsets;      // n + 1
    kgpu_span *spans; uint64_t span_cap;   // no store at or behind span_cap
};
int launch_source_spans(const SpansArgs &a, void *stream);
// The model inputs of a batch's ragged ids (kgpu_pack.hip; include/kanpyo_gpu.h, "model inputs"): padded rows [R, max_length] of ids, type ids, mask and,
// when asked for, spans and token indices.  b: n, sent_len (each sample's rows, then their offsets), text_offsets (the caller's row_offsets) and host_ctl
// ([0] the rows, [1] an input range out of bounds) alone are used.
struct PackArgs {
    RecordsBatch b;
    PackRule r;                        // kgpu_pack_core.h: the options, and whether the samples are pairs
    const int32_t *ids_a, *ids_b;     // n_ids_in entries each (ids_b: pairs only)
    const uint64_t *off_a, *off_b;     // n + 1 each
    uint64_t n_ids_in;
    const kgpu_span *spans_in;         // n_ids_in entries, or null
    const int32_t *tix_in;             // n_ids_in entries, or null
    int32_t *input_ids, *type_ids, *mask, *tix;   // row_cap x max_length each; all but input_ids may be null
    kgpu_span *spans;                  // row_cap x max_length, or null
    uint64_t row_cap;                  // nothing is stored when sent_len[n] > row_cap
    uint8_t *status;                   // n
};
int launch_pack(const PackArgs &a, void *stream);
// kgpu_pack_rule.cpp (HIP-free, compiles alone): rule 6 of "model inputs" for both forms of the call -> KGPU_OK, or KGPU_ERR_INVALID_ARG with the error set
int pack_check_args(const char *who, const kgpu_pack_opts *o, uint64_t n, const void *ids_a, const void *off_a, const void *ids_b, const void *off_b,
                    uint64_t n_ids_in, const void *spans_in, const void *tix_in, const void *input_ids, const void *type_ids, const void *mask,
                    const void *spans, const void *tix, uint64_t row_capacity, const void *row_offsets, const void *status);
// kgpu_normalize_table.cpp (HIP-free, compiles alone): the tables in host memory, their sizes in bytes, and one line on the host -> its status; out_len is
// the normalised length, and the bytes are in `out` when they fit `capacity` (the line itself where the status is not KGPU_SENT_OK)
struct NormTableSizes { size_t stage1, stage2, dec, pool, comp_key, comp_val; };
NormTables norm_host_tables();
NormTableSizes norm_table_sizes();
uint8_t norm_line_host(uint32_t form, const uint8_t *s, uint32_t len, uint8_t *out, uint64_t capacity, uint64_t &out_len);
// ... and its edits: n_edits is their number, and text and edits are written when BOTH fit
uint8_t norm_line_host_aligned(uint32_t form, const uint8_t *s, uint32_t len, uint8_t *out, uint64_t capacity, uint64_t &out_len, kgpu_norm_edit *edits,
                               uint64_t edit_capacity, uint64_t &n_edits);

// The text from ids (kgpu_decode.hip; include/kanpyo_gpu.h, "text from ids"): one line per sequence of ids, the words of its kept elements joined by the
// rule of kgpu_decode_core.h.  A word is found through `entry` -- one uint32 per list entry: where its arena entry lies, in 8-byte units -- in the initial
// table's arena ({u32 length, u32 hash, the bytes padded to 8}).  b: n, sent_len (each line's bytes, then their offsets), text_offsets and host_ctl ([0]
// the bytes) alone are used.
struct DecodeArgs {
    RecordsBatch b;
    DecodeRule r;
    const int32_t *ids;                // 4-byte aligned
    const uint64_t *id_offsets;        // n + 1, or null: padded rows of `width` ids
    uint64_t width;
    const uint32_t *entry;             // r.n_words entries
    const uint8_t *arena;
    uint8_t *status;                   // n
    uint8_t *text; uint64_t text_cap;  // nothing is stored when sent_len[n] > text_cap
};
int launch_decode(const DecodeArgs &a, void *stream);
// kgpu_vocab_table.cpp (HIP-free): the id -> arena entry table of a list's byte-keyed table, from its slots (tag = hash << 32 | (arena entry / 8 + 1))
void build_decode_entries(const VocabTables &t, uint64_t n_words, std::vector<uint32_t> &entry);
// kgpu_decode_host.cpp (HIP-free, compiles alone): the argument rules of all three forms of the call -> KGPU_OK, or KGPU_ERR_INVALID_ARG with the error set.
// host_offsets: id_offsets lies in host memory and is looked at.
int decode_check_args(const char *who, const void *ids, const void *id_offsets, bool host_offsets, uint64_t n, uint64_t width, const kgpu_decode_opts *o,
                      uint32_t prefix_len, const void *text, uint64_t text_capacity, const void *text_offsets, const void *status);

int pool_workgroups_per_cu(uint32_t pool_bytes, uint32_t waves);
int window_workgroups_per_cu(uint32_t lds_bytes);
int window_team_workgroups_per_cu(uint32_t lds_bytes);

}  // namespace kgpu
