"""The pool kernel's reservation arithmetic (kanpyo_amd/csrc/kgpu_pool.hip: k_tokenize_pool, launch_tokenize_pool) and the estimate's steering
step (kanpyo_amd/csrc/kgpu_chain.cpp: chain_feedback), restated in plain Python.  Every line names the line it restates; nothing here imports the
library.  For a fresh dictionary handle and one batch, what the kernel decides about a sentence is a function of that sentence alone -- its bytes B,
its characters C and the (targets, predecessors) of every start position of its lattice -- so tests/pool_cases.py can say which sentences the kernel
holds, which it redoes and which it hands on BEFORE anything runs on a GPU, and tests/test_gpu_pool_limits.py can ask for the routing counters as
exact numbers.

`shape` reads (T, P) per start position off the naive lattice of oracle/pyref.py; `verdict` is the model; `steer` is the estimate's step."""

MAXM = 8                  # kgpu_pool.hip:43   trie matches buffered per start position
POOL_HDR = 16             # kgpu_pool.hip:69   the bitmap and the ticket in front of the pages
POOL_PAGES = 64           # kgpu_pool.hip:71
EST_SLACK = 768           # kgpu_pool.hip:60   KGPU_EST_SLACK
EST_Q8_FRESH = 64 * 256   # kgpu_chain.h:83    Steering::est_q8 of a fresh handle
TILE_DIM = 8              # kgpu_tilepack.h:43

HELD, REDONE, ROUTED_BEFORE_WALK, ROUTED_AFTER_WALK = "HELD", "REDONE", "ROUTED_BEFORE_WALK", "ROUTED_AFTER_WALK"
ROUTED_MATCHES = "ROUTED_MATCHES"   # a fifth, outside the reservation: a match the walk could not park (MAXM, 256 characters); only with prefix_chars

# KGPU_POOL strings (kgpu_chain.cpp:37-61: "<KiB>:<wavefronts>[:<max pages>]", max pages 64 when left out) as (pool_bytes, waves, max_pages);
# SMALL is the single-launch small call's shape (kgpu_kernels.hip:665: one wavefront on 64 KB, every page its own)
PLAN_SHIPPED = (40 * 1024, 4, 32)
PLAN_160 = (160 * 1024, 4, 64)
PLAN_SMALL = (64 * 1024, 1, 64)
POOL_ENV = {PLAN_SHIPPED: "40:4:32", PLAN_160: "160:4"}


def align_up(v, a):
    return (v + a - 1) & ~(a - 1)                                       # kgpu_pool.hip:63


def page_bytes(plan):
    pool_bytes, waves, _ = plan
    return ((pool_bytes - POOL_HDR) // POOL_PAGES) & (~7 if waves == 1 else ~15)   # kgpu_pool.hip:812


def pages_for(nbytes, page):
    return (nbytes + page - 1) // page                                  # kgpu_pool.hip:187 (the multiply-high is this division below 2^32 / page bytes)


def tile_groups(n):
    return (n + TILE_DIM - 1) // TILE_DIM                               # kgpu_tilepack.h:43


def tile_count(T, P):
    return tile_groups(T) * tile_groups(P)                              # kgpu_tilepack.h:44


def need1(B, C, MS=4):
    return align_up(B + 4, 4) + 22 * (C + 2) + 2 * align_up(C + 2, 4) + align_up(C * MAXM * MS, 16) + 32   # kgpu_pool.hip:266


def verdict(B, C, tp, plan, est_q8=EST_Q8_FRESH, MS=4, est_slack=EST_SLACK, prefix_chars=None):
    """tp: (T, P) for the start positions 0..C -- T nodes start there (EOS starts at C), P nodes end there (BOS ends at 0).
    prefix_chars (optional): per start position the character lengths of its dictionary prefixes, for parks_every_match.
    -> {need1, est, npg, need_emit, need_full, page, limit, verdict, one_load}; need_emit / need_full are None when the walk was never paid for."""
    _, waves, max_pages = plan
    page = page_bytes(plan)
    pool_cap = page * POOL_PAGES                                        # kgpu_pool.hip:229
    own_slice = waves == 1                                              # kgpu_pool.hip:185
    out = {"page": page, "limit": max_pages * page, "need_emit": None, "need_full": None, "need1": None, "est": None, "npg": None,
           "one_load": [B + tsh + 4 <= 256 for tsh in range(4)]}        # kgpu_pool.hip:238, by the text's alignment
    if B + 64 > pool_cap or B > 0xFFF0:                                 # kgpu_pool.hip:230
        out["verdict"] = ROUTED_BEFORE_WALK
        return out
    n1 = need1(B, C, MS)
    est = max(n1, ((B * est_q8) >> 8) + est_slack)                      # kgpu_pool.hip:267
    npg = POOL_PAGES if own_slice else pages_for(min(est, pool_cap + page), page)   # kgpu_pool.hip:269
    out.update(need1=n1, est=est, npg=npg)
    if (n1 > pool_cap) if own_slice else (npg > max_pages):             # kgpu_pool.hip:272
        out["verdict"] = ROUTED_BEFORE_WALK
        return out
    lds_bytes = npg * page                                              # kgpu_pool.hip:279
    if prefix_chars is not None and not parks_every_match(prefix_chars):   # kgpu_pool.hip:438: behind the walk, in front of the fit test -- no late count
        out["verdict"] = ROUTED_MATCHES
        return out
    assert len(tp) == C + 1
    N = 1 + sum(t for t, _ in tp)                                       # kgpu_pool.hip:453,457,462: BOS is node 0, nb[C] = 1 is EOS (:440)
    Nb = sum(p for _, p in tp)                                          # kgpu_pool.hip:458,463: boff[0] holds BOS (:442), nothing ends behind C
    NT = sum(tile_count(t, p) for t, p in tp)                           # kgpu_pool.hip:459,464
    off = align_up(B + 4, 4)                                            # kgpu_pool.hip:302
    off += 4 * 4 * (C + 2)                                              # kgpu_pool.hip:303-306  nb, boff, bfill, ebase
    off += 3 * 2 * (C + 2)                                              # kgpu_pool.hip:307-309  cbyte, uspan, cp16
    off += 2 * align_up(C + 2, 4)                                       # kgpu_pool.hip:311-312  ccat, mcnt
    mbytes = align_up(C * MAXM * MS, 16)                                # kgpu_pool.hip:313
    off = align_up(off, 8)                                              # kgpu_pool.hip:473
    off += 8 * (N + 1)                                                  # kgpu_pool.hip:474  node[]
    off += 4 * N                                                        # kgpu_pool.hip:476  nSid[]
    off = align_up(off, 8)                                              # kgpu_pool.hip:477
    off_emit_end = off                                                  # kgpu_pool.hip:478
    off += 8 * (Nb + 1)                                                 # kgpu_pool.hip:479  bk[]
    need_emit, need_full = off_emit_end + mbytes + 16, off + 8 * NT     # kgpu_pool.hip:483
    out.update(need_emit=need_emit, need_full=need_full, N=N, Nb=Nb, NT=NT, lds_bytes=lds_bytes)
    if need_emit > lds_bytes or need_full > lds_bytes:                  # kgpu_pool.hip:484: late_count + 1 (:487)
        routed = pages_for(max(need_emit, need_full), page) > max_pages   # kgpu_pool.hip:489 (attempt is 0: the second attempt has the exact size)
        out["verdict"] = ROUTED_AFTER_WALK if routed else REDONE
        out["npg_redo"] = pages_for(max(need_emit, need_full), page)    # kgpu_pool.hip:490
    else:
        out["verdict"] = HELD
    return out


def parks_every_match(prefix_chars):
    """prefix_chars: per start position the character lengths of its dictionary prefixes.  False: the walk finds a ninth prefix at one position or
    one of 256 characters or more, and the sentence is handed on after the walk without a redo (kgpu_pool.hip:367,370,438)."""
    return all(len(p) <= MAXM and all(n < 256 for n in p) for p in prefix_chars)


def counters(verdicts):
    """-> (deferred[0], redone[0]) of a batch of these verdicts: every hand-on is a deferral (kgpu_pool.hip:181), every reservation that proved too
    small a late count (:487), whether the redo then held the sentence or handed it on (:489)."""
    return (sum(v in (ROUTED_BEFORE_WALK, ROUTED_AFTER_WALK, ROUTED_MATCHES) for v in verdicts), sum(v in (REDONE, ROUTED_AFTER_WALK) for v in verdicts))


def steer(est_q8, late, n):
    """chain_feedback's step of the estimate (kgpu_chain.cpp:218-224), applied to the value the batch ran with."""
    est = est_q8
    if late * 4 > n:                                                    # kgpu_chain.cpp:220
        est += est // 4
    elif late * 32 > n:                                                 # kgpu_chain.cpp:221
        est += est // 16
    elif late * 100 < n:                                                # kgpu_chain.cpp:222
        est -= est // 128
    return min(max(est, 16 * 256), 1024 * 256)                          # kgpu_chain.cpp:223


def shape(pyref, pd, s):
    """-> (T, P) per start position 0..C, and the nodes, dp, pre of the naive lattice (its edges[q] holds what ends at q: BOS in edges[0]; EOS, which
    starts at C, in edges[C + 1])."""
    nodes, edges, dp, pre = pyref.lattice(pd, s)
    C = len(s)
    T = [0] * (C + 1)
    for n in nodes[1:-1]:
        T[n[3]] += 1
    T[C] += 1   # EOS starts at C
    P = [len(edges[q]) for q in range(C + 1)]
    return list(zip(T, P)), nodes, dp, pre


def verdict_of(pyref, pd, s, plan, est_q8=EST_Q8_FRESH, **kw):
    """The model over the naive lattice of sentence s."""
    return verdict(len(s.encode("utf-8")), len(s), shape(pyref, pd, s)[0], plan, est_q8, **kw)
