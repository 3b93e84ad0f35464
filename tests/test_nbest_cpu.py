"""N-best paths without a device (include/kanpyo_gpu.h, "N-best paths"): kgpu_nbest_host against a brute-force enumeration of every path
(tests/nbest_ref.py) over the naive restatement's lattices (oracle/pyref.py), its first path against the oracle's tokens, its protocol, and the
surface of the feature -- header, binding, command line."""
import ctypes as C
import os

import numpy as np
import pytest

import nbest_ref as R
from conftest import ROOT, fixture_dict_parts
from dict_cases import lattice_from_pyref
from kanpyo_amd import _lib, cli
from kanpyo_amd.nbest import connection_matrix, lattice_struct, nbest_host
from nbest_cases import FIXTURE_INPUTS, conn_get_of, max_candidates, pydict_of, tie_case

INVALID, CAPACITY = _lib.KGPU_ERR_INVALID_ARG, _lib.KGPU_ERR_CAPACITY
N_TIE_CASES = 320


def _same(got, want):
    tokens, toff, costs = got
    wt, wo, wc = want[:3]
    assert costs.tolist() == wc.tolist() and toff.tolist() == wo.tolist()
    assert tokens.tobytes() == wt.astype(tokens.dtype).tobytes()


# ---- 1. the host function against brute force ------------------------------------------------------------------------------------------------------------
def test_fixture_dictionary_against_brute_force():
    from kanpyo_amd.dict import Dict

    d = Dict.from_parts(**fixture_dict_parts())
    pd, get = pydict_of(d), conn_get_of(d)
    n_paths = {}
    for s in FIXTURE_INPUTS:
        lat = lattice_from_pyref(pd, s)
        for k in (1, 2, 5, 64):
            got = nbest_host(lat, d, k)
            _same(got, R.first_k(lat, get, k))
            n_paths[s, k] = len(got[2])
    assert n_paths["", 64] == 1 and nbest_host(lattice_from_pyref(pd, ""), d, 3)[2].tolist() == [get(0, 0)]   # "": [EOS], cost M[0][0]
    assert 0 in n_paths.values()                                   # an unreachable EOS among them: no paths
    assert any(1 < n_paths[s, 64] < 64 for s in FIXTURE_INPUTS)    # fewer than k paths: all of them


def test_tie_dictionaries_against_brute_force():
    ties = 0
    ks = set()
    for seed in range(N_TIE_CASES):
        d, s, k = tie_case(seed)
        lat = lattice_from_pyref(pydict_of(d), s)
        want = R.first_k(lat, conn_get_of(d), k)
        _same(nbest_host(lat, d, k), want)
        ties += want[3]
        ks.add(k)
    assert ties * 3 >= N_TIE_CASES, ties     # the tie rule is really exercised
    assert len(ks) == 6


def test_more_than_64_candidates_against_brute_force():
    """A target with more candidates than one round of the device's selection holds, on the host: the tie dictionaries at k = 64."""
    seen = 0
    for seed in range(40):
        d, _, _ = tie_case(seed)
        s = "あいうえあいう"[: 5 + seed % 3]
        lat = lattice_from_pyref(pydict_of(d), s)
        if max_candidates(lat, 64)[1] > 64:
            seen += 1
            _same(nbest_host(lat, d, 64), R.first_k(lat, conn_get_of(d), 64))
    assert seen >= 10


# ---- 2. path 0 is the oracle's path -----------------------------------------------------------------------------------------------------------------------
def test_path_0_is_the_oracles_on_the_synthetic_corpus(oracle_mod):
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=11)
    pd, get = pydict_of(sd.dict), conn_get_of(sd.dict)
    orc = oracle_mod.OracleTokenizer.from_dict(sd.dict)
    conn = connection_matrix(sd.dict)
    for s in synth.make_corpus(sd, 200, 31, "cfg2"):
        lat = lattice_from_pyref(pd, s)
        tokens, toff, costs = nbest_host(lat, conn, 5)
        assert len(costs) >= 1
        assert tokens[: int(toff[1])].tobytes() == orc.tokenize(s)[0].tobytes(), s
        assert (np.diff(costs.astype(np.int64)) >= 0).all()
        paths = [tokens[int(toff[p]) : int(toff[p + 1])] for p in range(len(costs))]
        assert len({p.tobytes() for p in paths}) == len(paths)
        # each path's cost, recomputed from its records: the node of a record is found by its fields (a surface's duplicates differ in id)
        by_rec = {(n.id, int(n.class_), n.char_pos): n for n in lat.nodes[1:-1]}
        for p, path in enumerate(paths):
            chain = [lat.nodes[0]] + [by_rec[int(t["id"]), int(t["cls"]), int(t["start"])] for t in path[:-1]] + [lat.nodes[-1]]
            assert sum(b.cost + get(a.right_id, b.left_id) for a, b in zip(chain, chain[1:])) == int(costs[p])


# ---- 3. the protocol --------------------------------------------------------------------------------------------------------------------------------------
def _raw(lat_struct, conn, rows, cols, k, tcap, pcap, fill=0x5A):
    tokens = np.full((tcap + 2) * 24, fill, dtype=np.uint8)
    toff = np.full(pcap + 3, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    costs = np.full(pcap + 2, 0x5A5A5A5A, dtype=np.int32)
    P, T = C.c_uint64(77), C.c_uint64(77)
    rc = _lib.lib().kgpu_nbest_host(C.byref(lat_struct), conn.ctypes.data, rows, cols, k, tokens.ctypes.data, tcap, toff.ctypes.data, costs.ctypes.data, pcap,
                                    C.byref(P), C.byref(T))
    return rc, tokens, toff, costs, P.value, T.value


def test_protocol():
    d, _, _ = tie_case(3)
    lat = lattice_from_pyref(pydict_of(d), "あいうえあ")
    conn, rows, cols = connection_matrix(d)
    ls, keep = lattice_struct(lat)
    for k in (0, 65):
        rc, *_ = _raw(ls, conn, rows, cols, k, 100, 100)
        assert rc == INVALID and b"n_best" in _lib.lib().kgpu_last_error()
    want_t, want_o, want_c = nbest_host(lat, d, 8)
    P, T = len(want_c), len(want_t)
    assert P == 8 and T > P
    for tcap, pcap in ((T - 1, P), (T, P - 1), (0, 0)):   # one short: the exact sizes, nothing written
        rc, tokens, toff, costs, p, t = _raw(ls, conn, rows, cols, 8, tcap, pcap)
        assert rc == CAPACITY and (p, t) == (P, T)
        assert (tokens == 0x5A).all() and (toff == 0x5A5A5A5A5A5A5A5A).all() and (costs == 0x5A5A5A5A).all()
    rc, tokens, toff, costs, p, t = _raw(ls, conn, rows, cols, 8, T, P)   # an exact fit
    assert rc == _lib.KGPU_OK and (p, t) == (P, T)
    assert tokens[: T * 24].tobytes() == want_t.tobytes() and (tokens[T * 24 :] == 0x5A).all()
    assert toff[: P + 1].tolist() == want_o.tolist() and (toff[P + 1 :] == 0x5A5A5A5A5A5A5A5A).all()
    assert costs[:P].tolist() == want_c.tolist() and (costs[P:] == 0x5A5A5A5A).all()
    del keep


def test_inconsistent_lattices_are_rejected():
    d, _, _ = tie_case(5)
    lat = lattice_from_pyref(pydict_of(d), "あいう")
    conn, rows, cols = connection_matrix(d)

    def rc_of(change, rows=rows, cols=cols):
        ls, keep = lattice_struct(lat)
        change(ls, keep)
        return _raw(ls, conn, rows, cols, 3, 1000, 64)[0]

    assert rc_of(lambda ls, keep: None) == _lib.KGPU_OK
    assert rc_of(lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes))) == INVALID            # an edge node out of range
    assert rc_of(lambda ls, keep: keep[2].__setitem__(1, len(lat.nodes) - 1)) == INVALID        # ... or behind the node it leads to
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "end_char", 0) or setattr(keep[0][1], "char_pos", 1)) == INVALID   # end_char < char_pos
    assert rc_of(lambda ls, keep: setattr(keep[0][2], "left_id", 3)) == INVALID                 # a context id outside the matrix
    assert rc_of(lambda ls, keep: setattr(keep[0][2], "right_id", -1)) == INVALID
    assert rc_of(lambda ls, keep: None, cols=2) == INVALID
    assert rc_of(lambda ls, keep: setattr(keep[0][1], "char_pos", 99)) == INVALID               # starts behind the last position
    assert rc_of(lambda ls, keep: setattr(ls, "n_nodes", 1)) == INVALID


# ---- 4. the surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_header_and_makefile():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "kanpyo_gpu.h"), encoding="utf-8").read()
    for s, nargs in (("kgpu_nbest_host", 12), ("kgpu_tokenize_batch_nbest", 14)):
        assert s in _lib.SYMBOLS and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs and s + "(" in header, s
    assert "N-best paths" in header and "#define KGPU_NBEST_MAX 64" in header and _lib.KGPU_NBEST_MAX == 64
    with open(os.path.join(ROOT, "kanpyo_amd", "csrc", "Makefile"), encoding="utf-8") as f:
        mk = f.read()
    assert mk.count("kgpu_nbest.hip") == 2 and "kgpu_nbest_host.cpp" in mk and "kgpu_nbest_batch.cpp" in mk and "kgpu_nbest_core.h" in mk
    import kanpyo_amd
    from kanpyo_amd.tokenizer import Tokenizer

    assert kanpyo_amd.nbest_host is nbest_host and "nbest_host" in kanpyo_amd.__all__ and "NBestPath" in kanpyo_amd.__all__
    assert callable(Tokenizer.tokenize_nbest) and callable(Tokenizer.tokenize_nbest_packed)


def test_cli_parses_nbest_and_refuses_the_device_split(capsys):
    a = cli.parse_args(["tokenize", "-c", "x.dict", "--nbest", "5"])
    assert (a.command, a.nbest, a.split, a.normalize) == ("tokenize", 5, "host", "none")
    a = cli.parse_args(["tokenize", "すもも", "--nbest", "64", "--normalize", "nfkc"])
    assert (a.input, a.nbest, a.normalize) == ("すもも", 64, "nfkc")
    assert cli.parse_args(["tokenize"]).nbest is None and cli.parse_args([]).nbest is None
    for bad in (["--nbest", "0"], ["--nbest", "65"], ["--nbest", "x"], ["--nbest", "3", "--split", "device"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["tokenize"] + bad)
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_args(["wakati", "--nbest", "3"])   # tokenize's option alone
