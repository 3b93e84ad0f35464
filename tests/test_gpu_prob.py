"""Lattice probabilities on the device (include/kanpyo_gpu.h, "lattice probabilities"): kgpu_tokenize_batch_marginals, kgpu_tokenize_batch_samples,
Tokenizer.tokenize_marginals* / tokenize_samples* and `python -m kanpyo_amd tokenize --marginal / --sample`.  The device must equal kgpu_marginals_host
and kgpu_samples_host applied to kgpu_lattice_dump of the same sentence, byte for byte: records, probs, on_best, offsets, log_z, best_logprob, costs and
status.  The host functions themselves are pinned to a brute-force enumeration in tests/test_prob_cpu.py; the dump is compared with the naive restatement's
lattice node for node, and these calls with the host rules over the restatement's lattices, in tests/test_gpu_lattice_sweep.py.  test_the_two_functions_alone comes first:
everything else rests on the device rounding kexp and klog as the host does."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, fixture_dict_parts
from prob_cases import FIXTURE_INPUTS, THETAS, WIDE_SENTENCES, tie_dict, tie_sentence, wide_dict, widths

pytestmark = pytest.mark.gpu

NO_SCRATCH = 2
MIN_PROBS = (0.0, 0.01, 0.5)
SWEEP = [(False, 0.0, th) for th in THETAS] + [(True, mp, th) for mp in MIN_PROBS for th in THETAS]   # (all_nodes, min_prob, theta)
SAMPLE_SWEEP = [(ns, seed, THETAS[(i + j) % 4]) for i, ns in enumerate((1, 3, 256)) for j, seed in enumerate((0, (1 << 63) + 5))]


def _tok(d):
    from kanpyo_amd import Tokenizer, _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return Tokenizer(d)


class Host:
    """The host rule over kgpu_lattice_dump, sentence after sentence -> the arrays of the batch calls (a sentence given as bytes is not UTF-8).  A
    sentence's lattice is dumped and converted once."""

    def __init__(self, tok, d):
        from kanpyo_amd.nbest import connection_matrix

        self.tok, self.conn, self.lats = tok, connection_matrix(d), {}

    def lattice(self, s):
        from kanpyo_amd.lattice import dump_lattice
        from kanpyo_amd.nbest import lattice_struct

        if s not in self.lats:
            lat = dump_lattice(self.tok, s)
            self.lats[s] = (lat, lattice_struct(lat))
        return self.lats[s]

    def marginals(self, sents, theta, all_nodes, min_prob):
        from kanpyo_amd import _lib
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        conn, rows, cols = self.conn
        tokens, probs, best, toff, lzs, bls, status = [], [], [], [0], [], [], []
        for s in sents:
            if isinstance(s, bytes):
                toff.append(toff[-1]); lzs.append(-np.inf); bls.append(-np.inf); status.append(1)
                continue
            lat, (ls, _) = self.lattice(s)
            cap = len(lat.nodes)
            t, p, b = np.zeros(cap, dtype=TOKEN_DTYPE), np.zeros(cap, dtype=np.float64), np.zeros(cap, dtype=np.uint8)
            lz, bl, T = C.c_double(0), C.c_double(0), C.c_uint64(0)
            _lib.check(_lib.lib().kgpu_marginals_host(C.byref(ls), conn.ctypes.data, rows, cols, theta, 1 if all_nodes else 0, min_prob, t.ctypes.data, cap, p.ctypes.data,
                                                      b.ctypes.data, C.byref(lz), C.byref(bl), C.byref(T)))
            tokens.append(t[: T.value]); probs.append(p[: T.value]); best.append(b[: T.value])
            toff.append(toff[-1] + T.value); lzs.append(lz.value); bls.append(bl.value); status.append(0)
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)   # noqa: E731
        return (cat(tokens, TOKEN_DTYPE), cat(probs, np.float64), cat(best, np.uint8), np.array(toff, dtype=np.uint64), np.array(lzs, dtype=np.float64),
                np.array(bls, dtype=np.float64), np.array(status, dtype=np.uint8))

    def samples(self, sents, ns, seed, theta, first_index=0):
        from kanpyo_amd import _lib
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        conn, rows, cols = self.conn
        tokens, poff, toff, costs, status = [], [0], [0], [], []
        for i, s in enumerate(sents):
            if isinstance(s, bytes):
                poff.append(poff[-1]); status.append(1)
                continue
            lat, (ls, _) = self.lattice(s)
            tcap = ns * (lat.nodes[-1].char_pos + 1)
            t, o, c = np.zeros(max(tcap, 1), dtype=TOKEN_DTYPE), np.zeros(ns + 1, dtype=np.uint64), np.zeros(ns, dtype=np.int32)
            P, T = C.c_uint64(0), C.c_uint64(0)
            _lib.check(_lib.lib().kgpu_samples_host(C.byref(ls), conn.ctypes.data, rows, cols, theta, ns, seed, first_index + i, t.ctypes.data, tcap, o.ctypes.data, c.ctypes.data,
                                                    ns, C.byref(P), C.byref(T)))
            tokens.append(t[: T.value])
            toff += (o[1 : P.value + 1].astype(np.int64) + toff[-1]).tolist()
            costs += c[: P.value].tolist()
            poff.append(poff[-1] + P.value); status.append(0)
        return (np.concatenate(tokens) if tokens else np.zeros(0, dtype=TOKEN_DTYPE), np.array(poff, dtype=np.uint64), np.array(toff, dtype=np.uint64),
                np.array(costs, dtype=np.int32), np.array(status, dtype=np.uint8))


def _marginals(tok, sents, theta, all_nodes, min_prob):
    from kanpyo_amd.tokenizer import pack_sentences

    return tok.tokenize_marginals_packed(*pack_sentences(sents), theta, all_nodes, min_prob)


def _samples(tok, sents, ns, seed, theta):
    from kanpyo_amd.tokenizer import pack_sentences

    return tok.tokenize_samples_packed(*pack_sentences(sents), ns, seed, theta)


M_NAMES = ("tokens", "probs", "on_best", "tok_offsets", "log_z", "best_logprob", "status")
S_NAMES = ("tokens", "path_offsets", "tok_offsets", "costs", "status")


def _equal(got, want, names, what=""):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def _sweep(tok, host, sents, what=""):
    for all_nodes, mp, theta in SWEEP:
        _equal(_marginals(tok, sents, theta, all_nodes, mp), host.marginals(sents, theta, all_nodes, mp), M_NAMES, (what, all_nodes, mp, theta))
    for ns, seed, theta in SAMPLE_SWEEP:
        _equal(_samples(tok, sents, ns, seed, theta), host.samples(sents, ns, seed, theta), S_NAMES, (what, ns, seed, theta))


@pytest.fixture(scope="module")
def fixture_tok():
    from kanpyo_amd import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    tok = _tok(d)
    return d, tok, Host(tok, d)


@pytest.fixture(scope="module")
def wide_tok():
    d = wide_dict()
    tok = _tok(d)
    return d, tok, Host(tok, d)


# ---- 1. the two functions alone: FIRST -- a host / device arithmetic difference shows here and nowhere else ----------------------------------------------
def test_the_two_functions_alone():
    from kanpyo_amd import _lib
    from kanpyo_amd.prob import kexp_host, klog_host

    L = _lib.lib()
    assert L.kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    rng = np.random.default_rng(2040)
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    xe = np.concatenate([-32.0 * rng.random(40_000), -rng.exponential(1.0, 25_536), [0.0, -0.0, -32.0, np.nextafter(-32.0, -40.0), -33.0, -np.inf, -1e-300, -np.log(2.0)],
                         -np.arange(1, 33, dtype=np.float64)])
    xl = np.concatenate([np.exp(rng.uniform(-708.0, 709.0, 30_000)), rng.uniform(0.5, 2.0, 20_000), rng.uniform(1.0, 2.0**24, 15_536), 2.0 ** np.arange(-1022, 1024),
                         [tiny, big, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1.0 - 2.0**-53, 1.5, np.nextafter(1.5, 0.0)], 1.0 + np.arange(33) / 32.0])
    for which, x, host in ((0, xe, kexp_host), (1, xl, klog_host)):
        x = np.ascontiguousarray(x)
        out = np.zeros_like(x)
        _lib.check(L.kgpu_debug_prob_device(0, which, x.ctypes.data, x.size, out.ctypes.data))
        want = host(x)
        differ = np.flatnonzero(out.view(np.uint64) != want.view(np.uint64))
        print("kexp" if which == 0 else "klog", "arguments:", x.size, "differing:", differ.size, [(float(x[i]), float(out[i]), float(want[i])) for i in differ[:5]])
        assert differ.size == 0


# ---- 2. the device equals the host ------------------------------------------------------------------------------------------------------------------------
def test_fixture_sentences(fixture_tok):
    d, tok, host = fixture_tok
    sents = FIXTURE_INPUTS[:3] + [b"\xe3\x81"] + FIXTURE_INPUTS[3:] + [b"\xff", ""]   # invalid UTF-8 between valid sentences
    _sweep(tok, host, sents)
    got = _marginals(tok, sents, THETAS[0], False, 0.0)
    counts = np.diff(got[3].astype(np.int64)).tolist()
    assert counts[0] == 1 and got[1][0] == 1.0 and got[6].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0]      # "": [EOS] with 1
    unreachable = [i for i, s in enumerate(sents) if isinstance(s, str) and np.isneginf(got[4][i])]
    assert unreachable and all(counts[i] == 0 and np.isneginf(got[5][i]) and got[6][i] == 0 for i in unreachable)   # no records, status OK
    assert all(np.isneginf(got[4][i]) and counts[i] == 0 for i in (3, 7))


def test_tie_dictionaries():
    rng = random.Random(2041)
    for seed in range(4):   # 4 dictionaries x 16 sentences
        d = tie_dict(1000 + seed)
        tok = _tok(d)
        sents = [tie_sentence(rng) for _ in range(16)]
        _sweep(tok, Host(tok, d), sents, (seed, sents))
        tok.close()


def test_wide_dictionary(wide_tok):
    """More than 128 predecessors and more than 128 successors at a position: three rounds in the forward and in the backward kernel."""
    d, tok, host = wide_tok
    sents = list(WIDE_SENTENCES)
    assert min(widths(host.lattice(sents[0])[0])) > 128
    _sweep(tok, host, sents)
    got = _marginals(tok, sents, THETAS[0], True, 0.0)
    assert np.diff(got[3].astype(np.int64)).tolist() == [len(host.lattice(s)[0].nodes) - 1 for s in sents]


def test_synthetic_dictionary():
    """Sentences with unknown-word nodes; and BEST's records are tokenize's own."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sd = synth.build_dict(20000, seed=11)
    tok = _tok(sd.dict)
    host = Host(tok, sd.dict)
    sents = synth.make_corpus(sd, 64, 51, "cfg2")
    _sweep(tok, host, sents)
    assert any(int(n.class_) == 2 for s in sents[:8] for n in host.lattice(s)[0].nodes)
    utf8, offs = pack_sentences(sents)
    t1, toff1, st1 = tok.tokenize_packed(utf8, offs)
    got = tok.tokenize_marginals_packed(utf8, offs)
    assert got[0].tobytes() == t1.tobytes() and got[3].tolist() == toff1.tolist() and not got[6].any() and got[2].all()
    assert ((got[1] > 0) & (got[1] <= 1)).all() and (got[5] <= 0).all()
    # the Python classes
    rows = tok.tokenize_marginals(sents[:3] + [""])
    assert [[t for t, _, _ in r] for r in rows] == [list(r) for r in tok.tokenize_batch(sents[:3] + [""])] and rows[3][0][1] == 1.0
    paths = tok.tokenize_samples(sents[:3], 5, seed=9)
    assert all(len(p) == 5 for p in paths) and paths == tok.tokenize_samples(sents[:3], 5, seed=9) and paths != tok.tokenize_samples(sents[:3], 5, seed=10)
    tok.close()


# ---- 3. order, chunks, arena -------------------------------------------------------------------------------------------------------------------------------
def _per_sentence(got, n):
    """The marginals call's arrays cut by sentence."""
    toff = got[3].astype(np.int64)
    return [(got[0][toff[i] : toff[i + 1]].tobytes(), got[1][toff[i] : toff[i + 1]].tobytes(), got[2][toff[i] : toff[i + 1]].tobytes(), got[4][i].tobytes(),
             got[5][i].tobytes(), int(got[6][i])) for i in range(n)]


def test_order_independence(wide_tok):
    d, tok, host = wide_tok
    sents = ["あ" * k for k in (6, 1, 5, 2, 4, 3)]
    a, b = _marginals(tok, sents, 0.01, True, 0.0), _marginals(tok, sents, 0.01, True, 0.0)
    _equal(a, b, M_NAMES)
    rev = _marginals(tok, sents[::-1], 0.01, True, 0.0)
    assert _per_sentence(a, 6) == _per_sentence(rev, 6)[::-1]
    _equal(_samples(tok, sents, 16, 3, 0.01), _samples(tok, sents, 16, 3, 0.01), S_NAMES)


def test_chunking_gives_the_same_arrays(fixture_tok, monkeypatch):
    d, tok, host = fixture_tok
    sents = (FIXTURE_INPUTS + [b"\xff"] + FIXTURE_INPUTS[::-1])[:10]
    assert len(sents) == 10
    monkeypatch.delenv("KGPU_HOST_PROB_CHUNK_SENTS", raising=False)
    one_m, one_s = _marginals(tok, sents, THETAS[0], True, 0.0), _samples(tok, sents, 3, 11, THETAS[0])
    _equal(one_s, host.samples(sents, 3, 11, THETAS[0]), S_NAMES)
    monkeypatch.setenv("KGPU_HOST_PROB_CHUNK_SENTS", "3")
    _equal(_marginals(tok, sents, THETAS[0], True, 0.0), one_m, M_NAMES)
    _equal(_samples(tok, sents, 3, 11, THETAS[0]), one_s, S_NAMES)   # the hash takes the sentence's index in the call, not in its chunk


def test_arena_retry(wide_tok, monkeypatch):
    """The kept lattices and their slabs outgrow the arena: the chunk runs again on a doubled one and gives the same bytes."""
    d, tok, host = wide_tok
    sents = list(WIDE_SENTENCES) * 2
    want_m, want_s = _marginals(tok, sents, 0.01, True, 0.0), _samples(tok, sents, 64, 5, 0.01)
    monkeypatch.setenv("KGPU_HOST_PROB_ARENA_INITIAL", "16384")
    tok.routing(reset=True)
    _equal(_marginals(tok, sents, 0.01, True, 0.0), want_m, M_NAMES)
    assert tok.routing()["arena_regrows"] >= 2
    _equal(_samples(tok, sents, 64, 5, 0.01), want_s, S_NAMES)


def test_arena_limit(fixture_tok, monkeypatch):
    """At the largest arena the chunk is halved until the sentence that alone does not fit is left with KGPU_SENT_NO_SCRATCH and no records, its
    neighbours' being what they always are."""
    d, tok, host = fixture_tok
    long_ = "辞書形態素あ" * 25
    sents = FIXTURE_INPUTS + [long_] + FIXTURE_INPUTS[::-1]
    short = [s for s in sents if s != long_]
    want_m, want_s = _marginals(tok, short, THETAS[0], True, 0.0), _samples(tok, short[:6], 3, 1, THETAS[0])
    monkeypatch.setenv("KGPU_HOST_PROB_ARENA_INITIAL", "2048")
    monkeypatch.setenv("KGPU_HOST_PROB_ARENA_MAX", "8192")
    got = _marginals(tok, sents, THETAS[0], True, 0.0)
    assert got[6].tolist() == [0] * 6 + [NO_SCRATCH] + [0] * 6 and np.isneginf(got[4][6]) and got[3][6] == got[3][7]
    assert got[0].tobytes() == want_m[0].tobytes() and got[1].tobytes() == want_m[1].tobytes() and np.delete(got[3], 7).tolist() == want_m[3].tolist()
    assert np.delete(got[4], 6).tobytes() == want_m[4].tobytes()
    gs = _samples(tok, sents[:7], 3, 1, THETAS[0])   # (the sentences in front of the long one keep their indices in the call)
    assert gs[4].tolist() == [0] * 6 + [NO_SCRATCH] and gs[1][6] == gs[1][7] and gs[0].tobytes() == want_s[0].tobytes() and gs[3].tolist() == want_s[3].tolist()


def test_capacity_and_arguments(fixture_tok):
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import pack_sentences

    d, tok, host = fixture_tok
    utf8, offs = pack_sentences(FIXTURE_INPUTS)
    want = _marginals(tok, FIXTURE_INPUTS, 0.01, True, 0.0)
    T = len(want[0])
    with pytest.raises(_lib.KgpuError) as e:
        tok.tokenize_marginals_packed(utf8, offs, 0.01, True, 0.0, token_capacity=T - 1)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and str(T).encode() in _lib.lib().kgpu_last_error()
    _equal(tok.tokenize_marginals_packed(utf8, offs, 0.01, True, 0.0, token_capacity=T), want, M_NAMES)
    ws = _samples(tok, FIXTURE_INPUTS, 3, 2, 0.01)
    P, TS = len(ws[3]), len(ws[0])
    for kw in (dict(token_capacity=TS - 1, path_capacity=P), dict(token_capacity=TS, path_capacity=P - 1)):
        with pytest.raises(_lib.KgpuError) as e:
            tok.tokenize_samples_packed(utf8, offs, 3, 2, 0.01, **kw)
        assert e.value.code == _lib.KGPU_ERR_CAPACITY and str(TS).encode() in _lib.lib().kgpu_last_error() and str(P).encode() in _lib.lib().kgpu_last_error()
    _equal(tok.tokenize_samples_packed(utf8, offs, 3, 2, 0.01, token_capacity=TS, path_capacity=P), ws, S_NAMES)
    for call in (lambda: _marginals(tok, FIXTURE_INPUTS, 0.0, False, 0.0), lambda: _marginals(tok, FIXTURE_INPUTS, float("inf"), False, 0.0),
                 lambda: _marginals(tok, FIXTURE_INPUTS, float("nan"), False, 0.0), lambda: _marginals(tok, FIXTURE_INPUTS, 0.01, True, 1.5),
                 lambda: _marginals(tok, FIXTURE_INPUTS, 0.01, True, -0.5), lambda: _samples(tok, FIXTURE_INPUTS, 0, 0, 0.01),
                 lambda: _samples(tok, FIXTURE_INPUTS, 257, 0, 0.01), lambda: _samples(tok, FIXTURE_INPUTS, 3, 0, -1.0)):
        with pytest.raises(_lib.KgpuError) as e:
            call()
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG


# ---- 4. the command line -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_marginal_and_sample(fixture_tok, tmp_path):
    from conftest import load_golden
    from kanpyo_amd.dictfile import DictFile, MorphFeatureTable, save_dict
    from kanpyo_amd.nbest import path_lines
    from kanpyo_amd.prob import THETA_DEFAULT, marginal_lines, marginals_host, samples_host

    d, tok, host = fixture_tok
    g = load_golden("fixture_graphviz.json")
    p = fixture_dict_parts()
    known = MorphFeatureTable.from_features([g["features"]["known"].get(str(i), ["名詞", f"k{i}", "*"]) for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([g["features"]["unknown"][str(i)] for i in range(1, len(p["unk_morphs"]) + 1)])
    path = tmp_path / "t.dict"
    save_dict(DictFile(d, known, unk), str(path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    lines = [s for s in FIXTURE_INPUTS if s] + [g["input"]]
    data = "".join(s + "\n" for s in lines).encode()

    def run(extra, data=data):
        return subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)] + extra, input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)

    marg, samp = run(["--marginal"]), run(["--sample", "2", "--seed", "7"])
    assert marg.returncode == 0 and samp.returncode == 0, (marg.stderr, samp.stderr)
    want_m, want_s, reachable = b"", b"", []
    for i, s in enumerate(lines):
        lat = host.lattice(s)[0]
        t, pr, _, lz, _ = marginals_host(lat, d)
        want_m += marginal_lines(s.encode(), t, pr, known, unk)
        if np.isfinite(lz):
            reachable.append(s)
        t, o, c = samples_host(lat, d, 2, seed=7, sentence_index=i, theta=THETA_DEFAULT)
        want_s += b"".join(path_lines(s.encode(), t[int(o[q]) : int(o[q + 1])], known, unk) for q in range(len(c)))
    assert len(reachable) >= 3
    assert marg.stdout == want_m and marg.stdout.count(b"EOS\t\t1.000000\n") == len(reachable)
    assert samp.stdout == want_s and samp.stdout.count(b"EOS\t\n") == 2 * len(reachable)
    # --marginal with every probability column cut off is `tokenize` (on the lines whose EOS is reachable: the others have no distribution and print nothing)
    plain = run([], "".join(s + "\n" for s in reachable).encode())
    assert plain.returncode == 0 and b"".join(ln.rsplit(b"\t", 1)[0] + b"\n" for ln in marg.stdout.splitlines()) == plain.stdout
    bad = run(["--marginal", "--split", "device"])
    assert bad.returncode == 2 and bad.stdout == b""
