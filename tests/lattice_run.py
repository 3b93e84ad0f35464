"""What tests/test_gpu_lattice_sweep.py runs a dictionary through: the naive restatement's lattice of a sentence (oracle/pyref.py, as a
kanpyo_amd.lattice.Lattice), the device's dump compared with it node for node, and the arrays of every kept-lattice batch call -- graphviz, N-best,
marginals, samples, search / extended mode, user dictionary -- as the host rules give them over the RESTATEMENT's lattices, never over the dump.  A
sentence given as bytes is not UTF-8: no records, status 1.  Needs a device only where a Tokenizer is passed in, never at import; a mismatch names the
sentence and both records (tests/kernel_run.assert_records' style)."""
import numpy as np

from dict_cases import lattice_from_pyref
from nbest_cases import pydict_of

INF = 1 << 30
NBEST_NAMES = ("tokens", "path_offsets", "tok_offsets", "costs", "status")
MARGINAL_NAMES = ("tokens", "probs", "on_best", "tok_offsets", "log_z", "best_logprob", "status")
MODE_NAMES = ("tokens", "tok_offsets", "costs", "status")


def _name(s) -> str:
    return repr(s) if len(s) <= 80 else f"{s[:24]!r}... of {len(s)} characters"


class Ref:
    """One dictionary's restatement: its lattices (each sentence's made once) and the host rules over them."""

    def __init__(self, d):
        from kanpyo_amd.nbest import connection_matrix

        self.d, self.pd, self.conn, self._lat = d, pydict_of(d), connection_matrix(d), {}

    def lattice(self, s: str):
        if s not in self._lat:
            self._lat[s] = lattice_from_pyref(self.pd, s)
        return self._lat[s]

    # ---- the dump ---------------------------------------------------------------------------------------------------------------------------------
    def assert_dump(self, tok, s: str, what=""):
        """kgpu_lattice_dump of s on tok == the restatement's lattice: edges, then every field of every node."""
        from kanpyo_amd.lattice import dump_lattice

        got, want = dump_lattice(tok, s), self.lattice(s)
        if got.edges == want.edges and got.nodes == want.nodes:
            return
        pre = f"{what}: " if what else ""
        if len(got.nodes) != len(want.nodes):
            raise AssertionError(f"{pre}sentence {_name(s)}: the device has {len(got.nodes)} nodes, the restatement {len(want.nodes)}")
        for i, (g, w) in enumerate(zip(got.nodes, want.nodes)):
            if g != w:
                raise AssertionError(f"{pre}sentence {_name(s)}: node {i} differs: gpu {g} restatement {w}")
        e = next(k for k in range(max(len(got.edges), len(want.edges))) if got.edges[k : k + 1] != want.edges[k : k + 1])
        raise AssertionError(f"{pre}sentence {_name(s)}: the nodes ending at {e} differ: gpu {got.edges[e : e + 1]} restatement {want.edges[e : e + 1]}")

    # ---- the batch calls' arrays, by the host rules ---------------------------------------------------------------------------------------------
    def _paths(self, sents, one) -> tuple:
        """N-best's format from one(sentence index, lattice) -> (tokens, tok_offsets, costs) per sentence."""
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        tokens, poff, toff, costs, status = [], [0], [0], [], []
        for i, s in enumerate(sents):
            if isinstance(s, bytes):
                poff.append(poff[-1])
                status.append(1)
                continue
            t, o, c = one(i, self.lattice(s))
            tokens.append(t)
            toff += (o[1:].astype(np.int64) + toff[-1]).tolist()
            costs += c.tolist()
            poff.append(poff[-1] + len(c))
            status.append(0)
        return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(poff, dtype=np.uint64), np.array(toff, dtype=np.uint64),
                np.array(costs, dtype=np.int32), np.array(status, dtype=np.uint8))

    def nbest(self, sents, k: int) -> tuple:
        from kanpyo_amd.nbest import nbest_host

        seen = {}

        def one(_, lat):
            if id(lat) not in seen:
                seen[id(lat)] = nbest_host(lat, self.conn, k)
            return seen[id(lat)]
        return self._paths(sents, one)

    def samples(self, sents, n_samples: int, seed: int, theta: float) -> tuple:
        from kanpyo_amd.prob import samples_host

        return self._paths(sents, lambda i, lat: samples_host(lat, self.conn, n_samples, seed, i, theta))

    def marginals(self, sents, theta: float, all_nodes: bool, min_prob: float = 0.0) -> tuple:
        from kanpyo_amd.prob import marginals_host
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        tokens, probs, best, toff, lzs, bls, status, seen = [], [], [], [0], [], [], [], {}
        for s in sents:
            if isinstance(s, bytes):
                toff.append(toff[-1]); lzs.append(-np.inf); bls.append(-np.inf); status.append(1)
                continue
            if s not in seen:
                seen[s] = marginals_host(self.lattice(s), self.conn, theta, all_nodes, min_prob)
            t, p, b, lz, bl = seen[s]
            tokens.append(t); probs.append(p); best.append(b)
            toff.append(toff[-1] + len(t)); lzs.append(lz); bls.append(bl); status.append(0)
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)   # noqa: E731
        return (cat(tokens, TOKEN_DTYPE), cat(probs, np.float64), cat(best, np.uint8), np.array(toff, dtype=np.uint64), np.array(lzs, dtype=np.float64),
                np.array(bls, dtype=np.float64), np.array(status, dtype=np.uint8))

    def _records(self, sents, one) -> tuple:
        """The mode calls' format from one(sentence) -> (tokens, cost)."""
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        tokens, toff, costs, status, seen = [], [0], [], [], {}
        for s in sents:
            if isinstance(s, bytes):
                toff.append(toff[-1]); costs.append(INF); status.append(1)
                continue
            if s not in seen:
                seen[s] = one(s)
            t, c = seen[s]
            tokens.append(t)
            toff.append(toff[-1] + len(t)); costs.append(c); status.append(0)
        return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(toff, dtype=np.uint64), np.array(costs, dtype=np.int32),
                np.array(status, dtype=np.uint8))

    def mode(self, sents, mode, penalties=None) -> tuple:
        from kanpyo_amd.mode import mode_host

        return self._records(sents, lambda s: mode_host(self.lattice(s), s, self.conn, mode, penalties))

    def user(self, sents, entries, mode="normal", penalties=None) -> tuple:
        from kanpyo_amd.userdict import userdict_host

        return self._records(sents, lambda s: userdict_host(self.lattice(s), s, self.conn, self.d, entries, mode, penalties))

    def feature_tables(self) -> tuple:
        """Display tables for the graphviz call: one made-up feature list per record of the dictionary and per unknown record."""
        from kanpyo_amd.dictfile import MorphFeatureTable

        return (MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(self.pd.morphs) + 1)]),
                MorphFeatureTable.from_features([["未知語", "*", f"u{i}"] for i in range(1, len(self.pd.unk_morphs) + 1)]))

    def graphviz(self, sents, known, unk, dpi: int, full_state: bool) -> list:
        from kanpyo_amd.lattice import graphviz

        conn = lambda r, l: self.pd.conn[self.pd.row * l + r]  # noqa: E731  ConnectionTable::get (connection.rs:12-14)
        seen = {}
        for s in sents:
            if not isinstance(s, bytes) and s not in seen:
                seen[s] = graphviz(self.lattice(s), conn, known.features, unk.features, dpi, full_state).encode("utf-8")
        return [b"" if isinstance(s, bytes) else seen[s] for s in sents]


def assert_arrays(got, want, names, sents, what=""):
    """Whole arrays, byte for byte; the message names the first sentence whose share of the first differing array differs, where the array has one
    element per sentence or per sentence boundary."""
    for name, g, w in zip(names, got, want):
        if g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes():
            continue
        where = ""
        if g.shape == w.shape and len(g) in (len(sents), len(sents) + 1):
            i = max(int(np.nonzero(np.asarray(g != w))[0][0]) - (len(g) == len(sents) + 1), 0)
            where = f", first at sentence {i} ({_name(sents[i])}): gpu {g[i : i + 2].tolist()} host rule {w[i : i + 2].tolist()}"
        elif g.dtype == w.dtype and g.ndim == 1:
            n = min(len(g), len(w))
            bad = np.nonzero(np.asarray(g[:n] != w[:n]))[0]
            k = int(bad[0]) if bad.size else n
            where = f", first at element {k} of {len(g)} (the host rule has {len(w)}): gpu {g[k : k + 1].tolist()} host rule {w[k : k + 1].tolist()}"
        raise AssertionError(f"{what}: {name} differs ({g.dtype}{g.shape} against {w.dtype}{w.shape}){where}")


def device_docs(tok, sents, dpi: int, full_state: bool) -> tuple:
    """One graphviz call -> (the documents as bytes, status)."""
    from kanpyo_amd.tokenizer import pack_sentences

    text, toff, status = tok.graphviz_packed(*pack_sentences(sents), dpi=dpi, full_state=full_state)
    raw = text.tobytes()
    assert toff[0] == 0 and int(toff[-1]) == len(raw)
    return [raw[int(toff[i]) : int(toff[i + 1])] for i in range(len(sents))], status


def check_kept(tok, ref: Ref, sents, theta: float, penalties, what="", graphviz=True):
    """Every kept-lattice family over these sentences, ONE call each per setting, against the host rules over the restatement's lattices.  With k = 1,
    and with the marginals of the best path, the records are tokenize_packed's as well wherever the sentence has a real path.  -> calls made"""
    from kanpyo_amd.tokenizer import pack_sentences

    packed = pack_sentences(sents)
    bad = np.array([isinstance(s, bytes) for s in sents], dtype=bool)
    calls = 0
    if graphviz:
        known, unk = ref.feature_tables()
        tok.set_features(known, unk)
        for full_state in (True, False):
            docs, status = device_docs(tok, sents, 48, full_state)
            want = ref.graphviz(sents, known, unk, 48, full_state)
            assert status.tolist() == bad.astype(np.uint8).tolist(), (what, "graphviz status", full_state)
            for s, g, w in zip(sents, docs, want):
                assert g == w, f"{what}: graphviz(full_state={full_state}) of {_name(s)} differs"
            calls += 1
    plain, plain_off, plain_status = tok.tokenize_packed(*packed)
    assert plain_status.tolist() == bad.astype(np.uint8).tolist(), (what, "tokenize status")

    def same_as_plain(tokens, toff, real, name):
        for i in np.nonzero(real)[0]:
            a, b = tokens[int(toff[i]) : int(toff[i + 1])], plain[int(plain_off[i]) : int(plain_off[i + 1])]
            assert a.tobytes() == b.tobytes(), f"{what}: {name} of {_name(sents[i])} is not tokenize_packed's: {a.tolist()} against {b.tolist()}"

    for k in (1, 4, 64):
        got, want = tok.tokenize_nbest_packed(*packed, k), ref.nbest(sents, k)
        assert_arrays(got, want, NBEST_NAMES, sents, f"{what}: nbest k={k}")
        if k == 1:   # (at most one path per sentence: sentence i's is path number path_offsets[i])
            poff, toff = want[1].astype(np.int64), want[2].astype(np.int64)
            for i in np.nonzero(np.diff(poff) == 1)[0]:
                a, b = got[0][toff[poff[i]] : toff[poff[i] + 1]], plain[int(plain_off[i]) : int(plain_off[i + 1])]
                assert a.tobytes() == b.tobytes(), f"{what}: the best path of {_name(sents[i])} is not tokenize_packed's: {a.tolist()} against {b.tolist()}"
        calls += 1
    for all_nodes in (True, False):
        got, want = tok.tokenize_marginals_packed(*packed, theta, all_nodes, 0.0), ref.marginals(sents, theta, all_nodes)
        assert_arrays(got, want, MARGINAL_NAMES, sents, f"{what}: marginals all_nodes={all_nodes} theta={theta}")
        if not all_nodes:
            same_as_plain(got[0], got[3], np.isfinite(want[4]), "the best path's marginals")
        calls += 1
    assert_arrays(tok.tokenize_samples_packed(*packed, 3, 20241, theta), ref.samples(sents, 3, 20241, theta), NBEST_NAMES, sents, f"{what}: samples theta={theta}")
    for mode in ("normal", "search", "extended"):
        for pen in (None, penalties):
            assert_arrays(tok.tokenize_mode_packed(*packed, mode, pen), ref.mode(sents, mode, pen), MODE_NAMES, sents, f"{what}: mode {mode} {pen}")
            calls += 1
    return calls + 1


def check_user(tok, ref: Ref, sents, entries, modes=("normal", "search"), penalties=None, what="") -> dict:
    """tokenize_user_packed over these sentences in ONE call per mode == userdict_host over the restatement's lattices -> {mode: the device's arrays}."""
    from kanpyo_amd import UserDict
    from kanpyo_amd.tokenizer import pack_sentences

    ud = UserDict(tok, entries)
    out = {}
    try:
        for mode in modes:
            out[mode] = tok.tokenize_user_packed(*pack_sentences(sents), ud, mode, penalties)
            assert_arrays(out[mode], ref.user(sents, entries, mode, penalties), MODE_NAMES, sents, f"{what}: user dictionary, {mode}")
    finally:
        ud.close()
    return out
