"""A plain restatement of the search / extended mode rule (include/kanpyo_gpu.h, "search mode") over a kanpyo_amd.lattice.Lattice and its sentence:
the reference's forward as it is written (src/lattice.rs:116-142: a loop over the predecessors in their order, a strict '<'), with the penalty
added to the word cost, its backtrace, and the records.  Python ints and lists only; it imports nothing from the library.  The 64-bit keys, the
prefix counts of kanji and the wavefront minimum of kgpu_mode_core.h, kgpu_mode_host.cpp and kgpu_mode.hip are what it checks, so it has none of
them: a node's characters are looked at one by one."""
import dataclasses

import numpy as np

import nbest_ref as R

INF = 1 << 30
NORMAL, SEARCH, EXTENDED = 0, 1, 2
TOKEN_DTYPE = R.TOKEN_DTYPE


def is_kanji(ch: str) -> bool:
    cp = ord(ch)
    for lo, hi in ((0x3005, 0x3005), (0x3007, 0x3007), (0x3400, 0x4DBF), (0x4E00, 0x9FFF), (0xF900, 0xFAFF), (0x20000, 0x3FFFF)):
        if lo <= cp <= hi:
            return True
    return False


def penalty(node, text: str, mode: int, pen) -> int:
    kanji_length, kanji_penalty, other_length, other_penalty = pen
    if mode == NORMAL or int(node.class_) == 0:
        return 0
    chars = text[node.char_pos : node.end_char]
    assert len(chars) == node.end_char - node.char_pos
    if len(chars) > kanji_length and all(is_kanji(c) for c in chars):
        return min((len(chars) - kanji_length) * kanji_penalty, 1 << 29)
    if len(chars) > other_length:
        return min((len(chars) - other_length) * other_penalty, 1 << 29)
    return 0


def forward(lat, text: str, conn_get, mode: int, pen) -> tuple:
    """-> (dp, pre) per node: dp None for BOS (it counts 0), 1 << 30 where nothing was accepted."""
    nodes = lat.nodes
    dp, pre = [None] * len(nodes), [None] * len(nodes)
    for t in range(1, len(nodes)):   # (the reference walks the nodes by end position; a predecessor ends where its target starts, so any order that has it first gives the same)
        target = nodes[t]
        word = target.cost + penalty(target, text, mode, pen)
        dp[t] = INF
        for j in lat.edges[target.char_pos]:
            prev = 0 if dp[j] is None else dp[j]
            total = min(prev + word + conn_get(nodes[j].right_id, target.left_id), INF)
            assert -(1 << 31) <= prev + word + conn_get(nodes[j].right_id, target.left_id) < 1 << 31
            if total < dp[t]:
                dp[t], pre[t] = total, j
    return dp, pre


def chain(pre) -> list:
    """lattice.rs:144-153: from EOS along pre while there is one; the head is dropped."""
    pos, out = len(pre) - 1, []
    while pre[pos] is not None:
        out.append(pos)
        pos = pre[pos]
    return out[::-1]


def records(lat, text: str, path, mode: int) -> np.ndarray:
    rows = []
    starts = [0]
    for ch in text:
        starts.append(starts[-1] + len(ch.encode("utf-8")))
    for t in path:
        n = lat.nodes[t]
        if int(n.class_) == 0:
            rows.append((0, 0, n.byte_pos, n.char_pos, n.char_pos + 3, 0))
        elif mode == EXTENDED and int(n.class_) == 2 and n.end_char - n.char_pos > 1:
            rows += [(n.id, 2, starts[c], c, c + 1, starts[c + 1] - starts[c]) for c in range(n.char_pos, n.end_char)]
        else:
            rows.append((n.id, int(n.class_), n.byte_pos, n.char_pos, n.end_char, len(n.surface.encode("utf-8"))))
    out = np.zeros(len(rows), dtype=TOKEN_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def decode(lat, text: str, conn_get, mode: int, pen) -> tuple:
    """What kgpu_mode_host returns -> (tokens, cost)."""
    dp, pre = forward(lat, text, conn_get, mode, pen)
    return records(lat, text, chain(pre), mode), dp[-1]


def penalised(lat, text: str, mode: int, pen):
    """The lattice with every node's penalty in its word cost: a lattice whose plain best path is the mode's."""
    return dataclasses.replace(lat, nodes=[dataclasses.replace(n, cost=n.cost + penalty(n, text, mode, pen)) for n in lat.nodes])


def brute_force(lat, text: str, conn_get, mode: int, pen):
    """The minimum over every real BOS -> EOS path under the penalised costs, ties as tests/nbest_ref.py breaks them -> (tokens, cost), or None where
    EOS is unreachable."""
    paths = R.sorted_paths(penalised(lat, text, mode, pen), conn_get)
    if not paths:
        return None
    cost, path = paths[0]
    return records(lat, text, path, mode), cost
