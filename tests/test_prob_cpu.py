"""Lattice probabilities without a device (include/kanpyo_gpu.h, "lattice probabilities"): the two functions of the rule against numpy, kgpu_marginals_host
and kgpu_samples_host against a brute-force enumeration of every path (tests/prob_ref.py) over the naive restatement's lattices (oracle/pyref.py), the
protocol, the surface of the feature, and the host file under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import prob_ref as R
from conftest import ROOT, fixture_dict_parts
from dict_cases import lattice_from_pyref
from kanpyo_amd import _lib, cli
from kanpyo_amd.nbest import connection_matrix, lattice_struct, nbest_host
from kanpyo_amd.prob import THETA_DEFAULT, kexp_host, klog_host, marginals_host, samples_host
from nbest_cases import conn_get_of, pydict_of
from prob_cases import FIXTURE_INPUTS, THETAS, WIDE_SENTENCES, tie_case, wide_dict, widths

INVALID, CAPACITY = _lib.KGPU_ERR_INVALID_ARG, _lib.KGPU_ERR_CAPACITY
N_TIE_CASES = 300


# ---- 1. the two functions ----------------------------------------------------------------------------------------------------------------------------------
def test_kexp_accuracy():
    rng = np.random.default_rng(46)
    x = np.concatenate([-32.0 * rng.random(500_000), -rng.exponential(1.0, 500_000), [0.0, -0.0, -32.0, np.nextafter(-32.0, -40.0), -33.0, -1e300, -np.inf,
                        -1e-300, -2.0**-60, -math.log(2.0), -0.5 * math.log(2.0)], -np.arange(1, 33, dtype=np.float64)])
    got = kexp_host(x)
    want = np.where(x < -32.0, 0.0, np.exp(np.maximum(x, -745.0)))
    err = np.abs(got - want).max()
    print("kexp: largest absolute error", err)
    assert err <= 2.0**-46
    assert got[x < -32.0].tolist() == [0.0] * int((x < -32.0).sum()) and (got[x >= -32.0] > 0).all()
    assert kexp_host([0.0])[0] == 1.0 and kexp_host([-0.0])[0] == 1.0 and kexp_host([-32.0])[0] > 0 and kexp_host([np.nextafter(-32.0, -40.0)])[0] == 0.0


def test_klog_accuracy():
    rng = np.random.default_rng(47)
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    x = np.concatenate([np.exp(rng.uniform(-708.0, 709.0, 500_000)), rng.uniform(0.5, 2.0, 300_000), rng.uniform(1.0, 2.0**24, 200_000), 2.0 ** np.arange(-1022, 1024),
                        [tiny, np.nextafter(tiny, 1.0), big, np.nextafter(big, 0.0), 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1.0 - 2.0**-53, 1.5, np.nextafter(1.5, 0.0)],
                        1.0 + np.arange(33) / 32.0, np.nextafter(1.0 + np.arange(1, 33) / 32.0, 0.0)])
    got, want = klog_host(x), np.log(x)
    err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()
    print("klog: largest error over max(1, |log x|)", err)
    assert err <= 2.0**-46
    assert klog_host([1.0])[0] == 0.0 and klog_host([1.0 - 2.0**-53])[0] < 0 and klog_host([np.nextafter(1.0, 2.0)])[0] > 0


# ---- 2. the marginals against brute force ------------------------------------------------------------------------------------------------------------------
def _node_of(lat):
    """A record's node: by its fields (a surface's duplicates differ in id)."""
    by = {(n.id, int(n.class_), n.char_pos): t for t, n in enumerate(lat.nodes) if t}
    return lambda r: by[int(r["id"]), int(r["cls"]), int(r["start"])]


def _bound(lat, log_z):
    """B of the rule's error: per position one fix rounding per predecessor, the two functions' bounds and the additions -- (C + 2) positions."""
    chars = lat.nodes[-1].char_pos
    pmax = max(len(e) for e in lat.edges)
    return (chars + 2) * (pmax * 2.0**-41 + 2.0**-44 + abs(log_z) * 2.0**-50)


def _check_marginals(lat, d, get, theta):
    ex = R.Exact(lat, get, theta)
    tok_b, p_b, ob_b, lz, bl = marginals_host(lat, d, theta)
    tok_a, p_a, ob_a, lz_a, bl_a = marginals_host(lat, d, theta, all_nodes=True)
    assert (lz, bl) == (lz_a, bl_a)
    if not ex.reachable:
        assert lz == -math.inf and bl == -math.inf and len(tok_b) == 0 and len(tok_a) == 0
        return 0.0
    B = _bound(lat, ex.log_z)
    node = _node_of(lat)
    worst = abs(lz - ex.log_z) / B
    assert abs(lz - ex.log_z) <= B, (lz, ex.log_z, B)
    assert abs(bl - ex.best_logprob) <= 2 * B and bl <= 2 * B
    # the best selection: path 0 of N-best, EOS last with 1
    nb = nbest_host(lat, d, 1)
    assert tok_b.tobytes() == nb[0].tobytes() and ob_b.tolist() == [1] * len(tok_b) and p_b[-1] == 1.0
    # every node some path visits, in node order, each marginal within its bound
    listed = [node(r) for r in tok_a]
    assert listed == sorted(ex.marginal) and listed == sorted(listed)
    for t, p in zip(listed, p_a):
        assert abs(p - ex.marginal[t]) <= 4 * B + 2.0**-45, (t, p, ex.marginal[t])
        worst = max(worst, abs(p - ex.marginal[t]) / (4 * B + 2.0**-45))
    best_nodes = [node(r) for r in tok_b]
    assert [t for t, b in zip(listed, ob_a) if b] == best_nodes
    assert [float(p) for t, p in zip(listed, p_a) if t in best_nodes] == p_b.tolist()
    # a path covers every character once: the marginals of the nodes over a character sum to 1, and so do those of the nodes that start the sentence
    by_node = dict(zip(listed, p_a))
    for c in range(lat.nodes[-1].char_pos):
        total = math.fsum(p for t, p in by_node.items() if lat.nodes[t].char_pos <= c < lat.nodes[t].end_char)
        assert abs(total - 1.0) <= 4 * B + 2.0**-45, (c, total)
    if lat.nodes[-1].char_pos:
        assert abs(math.fsum(p for t, p in by_node.items() if lat.nodes[t].char_pos == 0) - 1.0) <= 4 * B + 2.0**-45
    # min_prob filters the same list
    half = marginals_host(lat, d, theta, all_nodes=True, min_prob=0.5)
    assert [node(r) for r in half[0]] == [t for t, p in zip(listed, p_a) if p >= 0.5] and half[1].tolist() == [float(p) for p in p_a if p >= 0.5]
    return worst


def test_marginals_of_the_tie_dictionaries_against_brute_force():
    worst, reach = 0.0, 0
    for seed in range(N_TIE_CASES):
        d, s = tie_case(seed)
        lat = lattice_from_pyref(pydict_of(d), s)
        get = conn_get_of(d)
        for theta in THETAS:
            worst = max(worst, _check_marginals(lat, d, get, theta))
        reach += math.isfinite(marginals_host(lat, d)[3])
    print("largest error as a share of its bound:", worst)
    assert reach >= N_TIE_CASES // 2


def test_marginals_of_the_fixture_dictionary():
    from kanpyo_amd.dict import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    pd, get = pydict_of(d), conn_get_of(d)
    lzs = []
    for s in FIXTURE_INPUTS:
        lat = lattice_from_pyref(pd, s)
        for theta in THETAS:
            _check_marginals(lat, d, get, theta)
        lzs.append(marginals_host(lat, d)[3])
    assert -math.inf in lzs and any(math.isfinite(z) for z in lzs)        # an unreachable EOS among them
    tok, p, ob, lz, bl = marginals_host(lattice_from_pyref(pd, ""), d)     # "": [EOS], one path
    assert len(tok) == 1 and p.tolist() == [1.0] and lz == -THETA_DEFAULT * get(0, 0) and bl == 0.0


def test_wide_dictionary_has_three_rounds_both_ways():
    d = wide_dict()
    lat = lattice_from_pyref(pydict_of(d), WIDE_SENTENCES[0])
    assert min(widths(lat)) > 128, widths(lat)
    tok, p, ob, lz, bl = marginals_host(lat, d, all_nodes=True)
    assert math.isfinite(lz) and len(tok) == len(lat.nodes) - 1 and abs(math.fsum(p[t - 1] for t in range(1, len(lat.nodes)) if lat.nodes[t].char_pos == 0) - 1.0) < 1e-9   # the nodes that start the sentence


# ---- 3. the samples ----------------------------------------------------------------------------------------------------------------------------------------
def _paths_of(lat, got):
    tokens, toff, costs = got
    node = _node_of(lat)
    return [(tuple(node(r) for r in tokens[int(toff[p]) : int(toff[p + 1])]), int(costs[p])) for p in range(len(costs))]


def test_samples_are_real_paths_with_their_costs():
    seen = 0
    for seed in range(60):
        d, s = tie_case(seed)
        lat = lattice_from_pyref(pydict_of(d), s)
        ex = R.Exact(lat, conn_get_of(d), 0.01)
        for ns, theta in ((1, THETA_DEFAULT), (3, 0.01), (256, 1.0)):
            got = samples_host(lat, d, ns, seed=seed, theta=theta)
            assert len(got[2]) == (ns if ex.reachable else 0) and len(got[1]) == len(got[2]) + 1
            for path, cost in _paths_of(lat, got):
                assert ex.cost[path] == cost
                seen += 1
    assert seen > 5000


def test_samples_are_a_function_of_seed_and_sentence_index():
    d, s = tie_case(3)
    lat = lattice_from_pyref(pydict_of(d), "あいうえあ")
    raw = lambda *a, **k: b"".join(x.tobytes() for x in samples_host(lat, d, *a, **k))   # noqa: E731
    base = raw(64, seed=5, sentence_index=2)
    assert raw(64, seed=5, sentence_index=2) == base
    assert raw(64, seed=6, sentence_index=2) != base and raw(64, seed=5, sentence_index=3) != base
    first = samples_host(lat, d, 8, seed=5, sentence_index=2)   # sample i does not depend on how many are drawn
    assert first[0].tobytes() == samples_host(lat, d, 64, seed=5, sentence_index=2)[0][: len(first[0])].tobytes()
    assert len(set(_paths_of(lat, samples_host(lat, d, 64, seed=5)))) > 1


def test_sample_frequencies_against_exact_probabilities():
    """20 seeded lattices of 2 to 40 paths, 79 calls of 256 draws each with consecutive seeds: every path's frequency within five standard deviations of
    its exact probability -- a cap against a broken sampler, not a measurement (the seeds are fixed: the test is deterministic)."""
    done, seed, worst = 0, 0, 0.0
    while done < 20:
        d, s = tie_case(seed)
        seed += 1
        lat = lattice_from_pyref(pydict_of(d), s)
        theta = THETAS[done % 2]
        ex = R.Exact(lat, conn_get_of(d), theta)
        if not 2 <= len(ex.paths) <= 40:
            continue
        count = {p: 0 for p in ex.prob}
        n = 0
        for call in range(79):
            for path, _ in _paths_of(lat, samples_host(lat, d, 256, seed=1000 * done + call, theta=theta)):
                count[path] += 1
                n += 1
        assert n == 79 * 256
        for path, p in ex.prob.items():
            sd = math.sqrt(p * (1 - p) / n)
            z = abs(count[path] / n - p) / sd if sd else 0.0
            worst = max(worst, z)
            assert abs(count[path] / n - p) <= 5 * sd + 1e-15, (done, path, count[path] / n, p, z)
        done += 1
    print("largest deviation in standard deviations:", worst)


# ---- 4. the protocol ---------------------------------------------------------------------------------------------------------------------------------------
def _raw_marginals(ls, conn, rows, cols, theta, select, min_prob, tcap):
    tokens, probs, best = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8), np.full(tcap + 2, 7.0), np.full(tcap + 2, 0x5A, dtype=np.uint8)
    lz, bl, T = C.c_double(5.0), C.c_double(5.0), C.c_uint64(77)
    rc = _lib.lib().kgpu_marginals_host(C.byref(ls), conn.ctypes.data, rows, cols, theta, select, min_prob, tokens.ctypes.data, tcap, probs.ctypes.data, best.ctypes.data,
                                        C.byref(lz), C.byref(bl), C.byref(T))
    return rc, tokens, probs, best, T.value


def _raw_samples(ls, conn, rows, cols, theta, ns, tcap, pcap):
    tokens, toff, costs = np.full((tcap + 2) * 24, 0x5A, dtype=np.uint8), np.full(pcap + 3, 7, dtype=np.uint64), np.full(pcap + 2, 7, dtype=np.int32)
    P, T = C.c_uint64(77), C.c_uint64(77)
    rc = _lib.lib().kgpu_samples_host(C.byref(ls), conn.ctypes.data, rows, cols, theta, ns, 1, 0, tokens.ctypes.data, tcap, toff.ctypes.data, costs.ctypes.data, pcap,
                                      C.byref(P), C.byref(T))
    return rc, tokens, toff, costs, P.value, T.value


def test_protocol():
    d, _ = tie_case(3)
    lat = lattice_from_pyref(pydict_of(d), "あいうえあ")
    conn, rows, cols = connection_matrix(d)
    ls, keep = lattice_struct(lat)
    last = _lib.lib().kgpu_last_error
    assert _raw_marginals(ls, conn, rows, cols, 2.0**64, 0, 0.0, 100)[0] == _lib.KGPU_OK and _lib.KGPU_THETA_MAX == 2.0**64   # the cap itself is a theta
    for theta in (0.0, -1.0, math.inf, math.nan, math.nextafter(2.0**64, math.inf), 1e300):
        assert _raw_marginals(ls, conn, rows, cols, theta, 0, 0.0, 100)[0] == INVALID and b"theta" in last()
        assert _raw_samples(ls, conn, rows, cols, theta, 1, 100, 100)[0] == INVALID and b"theta" in last()
    for mp in (-0.1, 1.5, math.nan):
        assert _raw_marginals(ls, conn, rows, cols, 0.01, 1, mp, 100)[0] == INVALID and b"min_prob" in last()
    assert _raw_marginals(ls, conn, rows, cols, 0.01, 2, 0.0, 100)[0] == INVALID and b"select" in last()
    for ns in (0, 257):
        assert _raw_samples(ls, conn, rows, cols, 0.01, ns, 100, 300)[0] == INVALID and b"n_samples" in last()
    want = marginals_host(lat, d, 0.01, all_nodes=True)
    T = len(want[0])
    rc, tokens, probs, best, t = _raw_marginals(ls, conn, rows, cols, 0.01, 1, 0.0, T - 1)   # one short: the exact size, no record written
    assert rc == CAPACITY and t == T and (tokens == 0x5A).all() and (probs == 7.0).all() and (best == 0x5A).all()
    rc, tokens, probs, best, t = _raw_marginals(ls, conn, rows, cols, 0.01, 1, 0.0, T)       # an exact fit
    assert rc == _lib.KGPU_OK and t == T and tokens[: T * 24].tobytes() == want[0].tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert probs[:T].tobytes() == want[1].tobytes() and (probs[T:] == 7.0).all() and best[:T].tolist() == want[2].tolist() and (best[T:] == 0x5A).all()
    wt, wo, wc = samples_host(lat, d, 8, seed=1, theta=0.01)
    P, T = len(wc), len(wt)
    assert P == 8
    for tcap, pcap in ((T - 1, P), (T, P - 1), (0, 0)):   # one short: both exact sizes, nothing written
        rc, tokens, toff, costs, p, t = _raw_samples(ls, conn, rows, cols, 0.01, 8, tcap, pcap)
        assert rc == CAPACITY and (p, t) == (P, T) and (tokens == 0x5A).all() and (toff == 7).all() and (costs == 7).all()
    rc, tokens, toff, costs, p, t = _raw_samples(ls, conn, rows, cols, 0.01, 8, T, P)
    assert rc == _lib.KGPU_OK and (p, t) == (P, T) and tokens[: T * 24].tobytes() == wt.tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert toff[: P + 1].tolist() == wo.tolist() and (toff[P + 1 :] == 7).all() and costs[:P].tolist() == wc.tolist() and (costs[P:] == 7).all()
    del keep


def test_inconsistent_lattices_are_rejected():
    d, _ = tie_case(5)
    lat = lattice_from_pyref(pydict_of(d), "あいう")
    conn, rows, cols = connection_matrix(d)

    def rcs(change, rows=rows, cols=cols):
        ls, keep = lattice_struct(lat)
        change(ls, keep)
        return _raw_marginals(ls, conn, rows, cols, 0.01, 1, 0.0, 1000)[0], _raw_samples(ls, conn, rows, cols, 0.01, 3, 1000, 64)[0]

    assert rcs(lambda ls, keep: None) == (_lib.KGPU_OK, _lib.KGPU_OK)
    bad = (INVALID, INVALID)
    assert rcs(lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes))) == bad            # an edge node out of range
    assert rcs(lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes) - 1)) == bad        # ... or behind the node it leads to
    assert rcs(lambda ls, keep: setattr(keep[0][1], "end_char", 0) or setattr(keep[0][1], "char_pos", 1)) == bad   # end_char < char_pos
    assert rcs(lambda ls, keep: setattr(keep[0][2], "left_id", 3)) == bad                 # a context id outside the matrix
    assert rcs(lambda ls, keep: setattr(keep[0][2], "right_id", -1)) == bad
    assert rcs(lambda ls, keep: None, cols=2) == bad
    assert rcs(lambda ls, keep: setattr(keep[0][1], "char_pos", 99)) == bad               # starts behind the last position
    assert rcs(lambda ls, keep: setattr(keep[0][1], "end_char", 99)) == bad               # ends behind it
    assert rcs(lambda ls, keep: setattr(keep[0][2], "pre", len(lat.nodes))) == bad        # a best predecessor that is not in front
    assert rcs(lambda ls, keep: setattr(ls, "n_nodes", 1)) == bad


# ---- 5. the surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_header_and_makefile():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "kanpyo_gpu.h"), encoding="utf-8").read()
    for s, nargs in (("kgpu_marginals_host", 14), ("kgpu_samples_host", 15), ("kgpu_tokenize_batch_marginals", 16), ("kgpu_tokenize_batch_samples", 16),
                     ("kgpu_prob_exp_host", 3), ("kgpu_prob_log_host", 3)):
        assert s in _lib.SYMBOLS and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs and s + "(" in header, s
    assert len(L.kgpu_debug_prob_device.argtypes) == 5 and "kgpu_debug_prob_device" not in _lib.SYMBOLS   # (a test-only export, as the other kgpu_debug_* are)
    assert "lattice probabilities" in header and "#define KGPU_SAMPLES_MAX 256" in header and _lib.KGPU_SAMPLES_MAX == 256
    assert "#define KGPU_MARGINAL_BEST 0u" in header and "#define KGPU_MARGINAL_ALL 1u" in header and "#define KGPU_THETA_MAX 18446744073709551616.0" in header and THETA_DEFAULT == 0.75 / 800
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_prob.hip") == 2 and "kgpu_prob_host.cpp" in mk and "kgpu_prob_batch.cpp" in mk and "kgpu_prob_core.h" in mk
    core = open(os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_prob_core.h"), encoding="utf-8").read()
    assert "#pragma clang fp contract(off)" in core and "<cmath>" not in core and "math.h" not in core
    import kanpyo_amd
    from kanpyo_amd.tokenizer import Tokenizer

    assert kanpyo_amd.marginals_host is marginals_host and kanpyo_amd.samples_host is samples_host and "marginals_host" in kanpyo_amd.__all__ and "samples_host" in kanpyo_amd.__all__
    for m in ("tokenize_marginals", "tokenize_marginals_packed", "tokenize_samples", "tokenize_samples_packed"):
        assert callable(getattr(Tokenizer, m)), m


def test_cli_parses_the_probability_options(capsys):
    a = cli.parse_args(["tokenize", "-c", "x.dict", "--marginal"])
    assert (a.command, a.marginal, a.all_morphs, a.min_prob, a.theta, a.sample, a.seed) == ("tokenize", True, False, 0.0, THETA_DEFAULT, None, 0)
    a = cli.parse_args(["tokenize", "すもも", "--marginal", "--all-morphs", "--min-prob", "0.01", "--theta", "0.5", "--normalize", "nfkc"])
    assert (a.input, a.marginal, a.all_morphs, a.min_prob, a.theta, a.normalize) == ("すもも", True, True, 0.01, 0.5, "nfkc")
    a = cli.parse_args(["tokenize", "--sample", "4", "--seed", "7", "--theta", "0.001"])
    assert (a.sample, a.seed, a.theta, a.marginal) == (4, 7, 0.001, False)
    assert cli.parse_args(["tokenize"]).sample is None and not cli.parse_args([]).marginal
    for bad in (["--sample", "0"], ["--sample", "257"], ["--sample", "x"], ["--sample", "3", "--split", "device"], ["--marginal", "--split", "device"],
                ["--marginal", "--nbest", "2"], ["--sample", "2", "--nbest", "2"], ["--marginal", "--sample", "2"], ["--marginal", "--theta", "0"],
                ["--marginal", "--theta", "inf"], ["--marginal", "--theta", "1e20"], ["--marginal", "--min-prob", "1.5"], ["--all-morphs"], ["--min-prob", "0.1"], ["--seed", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["tokenize"] + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_args(["wakati", "--marginal"])   # tokenize's options alone


# ---- 6. the host file under the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_host_functions_under_asan_ubsan(tmp_path):
    """A stand-alone program (tests/prob_sanitize_main.cpp, its own main) linked with kgpu_prob_host.cpp alone: nothing is loaded into Python."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):   # (the probe of tests/test_chartrie_sanitize.py, before any work)
        pytest.skip("no libasan in this toolchain")
    exe = str(tmp_path / "prob_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "prob_sanitize_main.cpp"), os.path.join(ROOT, "kanpyo_amd", "csrc", "kgpu_prob_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prob sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
