"""A plain restatement of the user dictionary rule (include/kanpyo_gpu.h, "user dictionary") over a kanpyo_amd.lattice.Lattice, its sentence and a list
of entries (surface, left_id, right_id, cost, ...): the matches by str.startswith at every character position, the withdrawn unknown nodes, the
reference's forward as it is written (a loop over the predecessors in ascending combined index, a strict '<') over the widened node set, its backtrace
and the records; and a brute-force enumerator of every path of the widened lattice.  Python ints, lists and strs only; it imports nothing from the
library.  The hash table, the length mask, the 64-bit keys, the counting sort and the wavefront minimum of kgpu_user_core.h, kgpu_user_host.cpp and
kgpu_user.hip are what it checks, so it has none of them."""
import functools
from collections import namedtuple

import numpy as np

import mode_ref as M

INF = 1 << 30
USER = 3
TOKEN_DTYPE = M.TOKEN_DTYPE

# a node of the widened set: the lattice's own (kind "lat", ref its index) or a user node (kind "user", ref the entry's index)
WNode = namedtuple("WNode", "kind ref cls start end left right cost")
Widened = namedtuple("Widened", "nodes preds withdrawn n_lattice")


def invoke_of(d, text: str) -> list:
    """Per character whether its category is in the Dict's invoke_list (a code point beyond the table has code point 0's category)."""
    cat, inv = d.char_category, d.invoke_list
    out = []
    for ch in text:
        c = int(cat[ord(ch)]) if ord(ch) < len(cat) else int(cat[0])
        out.append(bool(c < len(inv) and inv[c]))
    return out


def widen(lat, text: str, entries, invoke) -> Widened:
    """The lattice's nodes, then the user nodes by (q, e); per position the predecessors (combined indices, ascending) that are not withdrawn."""
    N, C = len(lat.nodes), len(text)
    nodes = [WNode("lat", i, int(n.class_), n.char_pos, n.end_char, n.left_id, n.right_id, n.cost) for i, n in enumerate(lat.nodes)]
    hit = [False] * (C + 1)
    for q in range(C):
        for e, ent in enumerate(entries):
            key = ent[0]
            if text.startswith(key, q):
                hit[q] = True
                nodes.append(WNode("user", e, USER, q, q + len(key), int(ent[1]), int(ent[2]), int(ent[3])))
    known_at = {n.char_pos for n in lat.nodes if int(n.class_) == 1}
    withdrawn = {i for i, n in enumerate(lat.nodes) if int(n.class_) == 2 and n.char_pos < C and hit[n.char_pos] and n.char_pos not in known_at and not invoke[n.char_pos]}
    preds = [[j for j in e if j not in withdrawn] for e in lat.edges]
    while len(preds) < C + 2:
        preds.append([])
    for i in range(N, len(nodes)):
        preds[nodes[i].end].append(i)
    return Widened(nodes, preds, withdrawn, N)


def penalty(node: WNode, text: str, mode: int, pen) -> int:
    kanji_length, kanji_penalty, other_length, other_penalty = pen
    if mode == M.NORMAL or node.cls == 0:
        return 0
    chars = text[node.start : node.end]
    if len(chars) > kanji_length and all(M.is_kanji(c) for c in chars):
        return min((len(chars) - kanji_length) * kanji_penalty, 1 << 29)
    if len(chars) > other_length:
        return min((len(chars) - other_length) * other_penalty, 1 << 29)
    return 0


def forward(w: Widened, text: str, conn_get, mode: int, pen) -> tuple:
    """-> (dp, pre) per node of the widened set; a withdrawn node keeps (None, None) and nothing looks at it."""
    dp, pre = [None] * len(w.nodes), [None] * len(w.nodes)
    order = sorted(range(1, len(w.nodes)), key=lambda i: (w.nodes[i].start, i))   # a predecessor ends where its target starts: it starts in front of it
    for t in order:
        if t in w.withdrawn:
            continue
        target = w.nodes[t]
        word = target.cost + penalty(target, text, mode, pen)
        dp[t] = INF
        for j in w.preds[target.start]:
            prev = 0 if dp[j] is None else dp[j]
            total = min(prev + word + conn_get(w.nodes[j].right, target.left), INF)
            if total < dp[t]:
                dp[t], pre[t] = total, j
    return dp, pre


def chain(w: Widened, pre) -> list:
    pos, out = w.n_lattice - 1, []
    while pre[pos] is not None:
        out.append(pos)
        pos = pre[pos]
    return out[::-1]


def records(w: Widened, lat, text: str, path, mode: int) -> np.ndarray:
    starts = [0]
    for ch in text:
        starts.append(starts[-1] + len(ch.encode("utf-8")))
    rows = []
    for t in path:
        n = w.nodes[t]
        if n.kind == "user":
            rows.append((n.ref + 1, USER, starts[n.start], n.start, n.end, starts[n.end] - starts[n.start]))
        else:
            rows += [tuple(int(r[f]) for f in TOKEN_DTYPE.names) for r in M.records(lat, text, [n.ref], mode)]
    out = np.zeros(len(rows), dtype=TOKEN_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def decode(lat, text: str, conn_get, entries, invoke, mode: int, pen) -> tuple:
    """What kgpu_userdict_host returns -> (tokens, cost)."""
    w = widen(lat, text, entries, invoke)
    dp, pre = forward(w, text, conn_get, mode, pen)
    return records(w, lat, text, chain(w, pre), mode), dp[w.n_lattice - 1]


# ---- every path ----------------------------------------------------------------------------------------------------------------------------------------------
MAX_PATHS = 200_000


def all_paths(w: Widened, text: str, conn_get, mode: int, pen) -> list:
    """Every real BOS -> EOS path of the widened lattice as (nodes, the cost up to and including each): a path one of whose prefixes costs 1 << 30 or
    more is no path.  None where there are more than MAX_PATHS."""
    eos = w.n_lattice - 1
    starts_at = {}
    for i, n in enumerate(w.nodes):
        if i and i not in w.withdrawn:
            starts_at.setdefault(n.start, []).append(i)
    out = []
    stack = [((0,), (0,))]
    while stack:
        path, costs = stack.pop()
        last = w.nodes[path[-1]]
        if path[-1] == eos:
            out.append((path, costs))
            if len(out) > MAX_PATHS:
                return None
            continue
        for t in starts_at.get(last.end, []):
            n = w.nodes[t]
            c = costs[-1] + n.cost + penalty(n, text, mode, pen) + conn_get(last.right, n.left)
            if c < INF:
                stack.append((path + (t,), costs + (c,)))
    return out


def _compare(a, b) -> int:
    """Two paths that end at the same node: cost, then the lower predecessor (combined index), then the prefixes."""
    (pa, ca), (pb, cb) = a, b
    k = 1
    while True:
        if ca[-k] != cb[-k]:
            return -1 if ca[-k] < cb[-k] else 1
        if len(pa) == k or len(pb) == k:
            return 0
        if pa[-k - 1] != pb[-k - 1]:
            return -1 if pa[-k - 1] < pb[-k - 1] else 1
        k += 1


def brute_force(lat, text: str, conn_get, entries, invoke, mode: int, pen):
    """The minimum over every real BOS -> EOS path of the widened lattice, ties as the rule breaks them -> (tokens, cost); None where EOS is unreachable
    (the forward's quirks decide there) or the paths are too many."""
    w = widen(lat, text, entries, invoke)
    paths = all_paths(w, text, conn_get, mode, pen)
    if not paths:
        return None
    path, costs = min(paths, key=functools.cmp_to_key(_compare))
    return records(w, lat, text, path[1:], mode), costs[-1]
