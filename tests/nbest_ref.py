"""A plain reference for the N-best paths (include/kanpyo_gpu.h, "N-best paths"): every BOS -> EOS path of a kanpyo_amd.lattice.Lattice, enumerated
and sorted with the rule's recursive comparator -- cost first, then (backwards from EOS) the lower predecessor node index, then the order of the two
prefixes.  Python lists and functools only; it imports nothing from the library.  The lists per node, the 64-bit keys and the selection networks of
kgpu_nbest_host.cpp and kgpu_nbest.hip are what it checks, so it has none of them."""
import functools

import numpy as np

INF = 1 << 30
MAX_PATHS = 200_000
# kgpu_token (include/kanpyo_gpu.h)
TOKEN_DTYPE = np.dtype([("id", "<i4"), ("cls", "<u4"), ("position", "<u4"), ("start", "<u4"), ("end", "<u4"), ("byte_len", "<u4")])


def count_paths(lat) -> int:
    """The BOS -> EOS paths of the lattice, by a DP over the nodes (a predecessor is in front of its target)."""
    cnt = [0] * len(lat.nodes)
    cnt[0] = 1
    for t in range(1, len(lat.nodes)):
        cnt[t] = sum(cnt[j] for j in lat.edges[lat.nodes[t].char_pos])
    return cnt[-1]


def all_paths(lat, conn_get) -> list:
    """Every real BOS -> EOS path as (nodes from BOS to EOS, the cost up to and including each of them): a path one of whose prefixes costs
    1 << 30 or more is no path (the rule drops that candidate).  conn_get(right_id, left_id) = ConnectionTable::get."""
    total = count_paths(lat)
    assert total <= MAX_PATHS, f"{total} paths: too many to enumerate"
    nodes = lat.nodes
    done = []
    stack = [[len(nodes) - 1]]   # chains from EOS backwards
    while stack:
        chain = stack.pop()
        if chain[-1] == 0:
            path = chain[::-1]
            costs, ok = [0], True
            for a, b in zip(path, path[1:]):
                costs.append(costs[-1] + nodes[b].cost + conn_get(nodes[a].right_id, nodes[b].left_id))
                ok = ok and costs[-1] < INF
            if ok:
                done.append((path, costs))
            continue
        for j in lat.edges[nodes[chain[-1]].char_pos]:
            stack.append(chain + [j])
    return done


def _compare(a, b) -> int:
    """Two paths that end at the same node: cost, then the lower predecessor index, then the prefixes."""
    (pa, ca), (pb, cb) = a, b
    k = 1
    while True:
        if ca[-k] != cb[-k]:
            return -1 if ca[-k] < cb[-k] else 1
        if k == len(pa) or k == len(pb):   # (one of them is down at BOS: both are, or the predecessors differed)
            return 0
        if pa[-k - 1] != pb[-k - 1]:
            return -1 if pa[-k - 1] < pb[-k - 1] else 1
        k += 1


def sorted_paths(lat, conn_get) -> list:
    """all_paths in the rule's order -> [(cost, nodes from the first word to EOS)]."""
    return [(c[-1], p[1:]) for p, c in sorted(all_paths(lat, conn_get), key=functools.cmp_to_key(_compare))]


def records_of(lat, path) -> np.ndarray:
    """The kgpu_token records tokenize emits for these nodes (tokenizer.rs:20-43: the EOS dummy is "EOS", three characters and no bytes)."""
    out = np.zeros(len(path), dtype=TOKEN_DTYPE)
    for i, t in enumerate(path):
        n = lat.nodes[t]
        if int(n.class_) == 0:
            out[i] = (0, 0, n.byte_pos, n.char_pos, n.char_pos + 3, 0)
        else:
            out[i] = (n.id, int(n.class_), n.byte_pos, n.char_pos, n.end_char, len(n.surface.encode("utf-8")))
    return out


def first_k(lat, conn_get, k: int) -> tuple:
    """What kgpu_nbest_host returns for n_best = k -> (tokens, tok_offsets, costs) -- and whether the first k + 1 paths hold a cost tie."""
    paths = sorted_paths(lat, conn_get)
    head = [c for c, _ in paths[: k + 1]]
    tie = len(set(head)) < len(head)
    paths = paths[:k]
    toff = np.zeros(len(paths) + 1, dtype=np.uint64)
    if paths:
        toff[1:] = np.cumsum([len(p) for _, p in paths])
    tokens = np.concatenate([records_of(lat, p) for _, p in paths]) if paths else np.zeros(0, dtype=TOKEN_DTYPE)
    return tokens, toff, np.array([c for c, _ in paths], dtype=np.int32), tie
