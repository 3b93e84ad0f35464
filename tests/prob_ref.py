"""A plain reference for the lattice probabilities (include/kanpyo_gpu.h, "lattice probabilities"): every BOS -> EOS path of a
kanpyo_amd.lattice.Lattice enumerated, its weight exp(-theta (cost - the lowest cost)), and every sum by math.fsum.  It imports nothing from the
library: the recursions, the fixed-point sums and the two functions of kgpu_prob_core.h are what it checks, so it has none of them."""
import math

MAX_PATHS = 200_000


def all_paths(lat, conn_get) -> list:
    """Every BOS -> EOS path -> [(nodes from the first word to EOS, cost)]."""
    nodes = lat.nodes
    cnt = [0] * len(nodes)
    cnt[0] = 1
    for t in range(1, len(nodes)):
        cnt[t] = sum(cnt[j] for j in lat.edges[nodes[t].char_pos])
    assert cnt[-1] <= MAX_PATHS, f"{cnt[-1]} paths: too many to enumerate"
    done, stack = [], [([len(nodes) - 1], 0)]   # chains from EOS backwards
    while stack:
        chain, cost = stack.pop()
        t = chain[-1]
        if t == 0:
            done.append((tuple(chain[-2::-1]), cost))
            continue
        for j in lat.edges[nodes[t].char_pos]:
            stack.append((chain + [j], cost + nodes[t].cost + conn_get(nodes[j].right_id, nodes[t].left_id)))
    return done


class Exact:
    """The distribution over the paths of a lattice at theta: log_z, each path's probability, each node's marginal, the best path's log-probability."""

    def __init__(self, lat, conn_get, theta: float):
        self.paths = all_paths(lat, conn_get)
        self.reachable = bool(self.paths)
        if not self.reachable:
            self.log_z = self.best_logprob = -math.inf
            self.marginal, self.prob = {}, {}
            return
        cmin = min(c for _, c in self.paths)
        w = [math.exp(-theta * (c - cmin)) for _, c in self.paths]
        z = math.fsum(w)
        self.log_z = -theta * cmin + math.log(z)
        self.best_logprob = -math.log(z)   # the lowest cost is tokenize's: -theta cmin - log_z
        self.prob = {}
        per_node = {}
        for (p, _), wi in zip(self.paths, w):
            self.prob[p] = self.prob.get(p, 0.0) + wi / z   # (a path is its node tuple: no two paths share one)
            for t in p:
                per_node.setdefault(t, []).append(wi)
        self.marginal = {t: math.fsum(ws) / z for t, ws in per_node.items()}
        self.cost = dict(self.paths)
