"""GPU parity on connection matrices that are not square, context ids that are not plain (row, col) pairs and costs at the
i16 extremes (synth.matrix_case, tests/test_matrix_cpu.py's hand dictionaries).  ConnectionTable::get(right, left) =
data[rows * left + right] (connection.rs:12-14): the runtime ranks the ids of a dictionary whose ids are plain pairs
and both axes below 65 536, and keeps them as they are otherwise (kgpu_dict.cpp); every kernel indexes the matrix by
rows alone, packs ids and costs into 16-bit fields, and clamps at INF (lattice.rs:116-150).  Each launch path against
the oracle, exact equality."""
import itertools
import random

import numpy as np
import pytest

from conftest import fixture_dict_parts
from dict_cases import lattice_from_pyref, saturation_parts, transposed_parts
from kernel_cases import CHAIN_KNOBS
from kernel_run import STATUS_MARKER, assert_records, device_batch, host_batch, libs, set_env  # noqa: F401  (libs: the fixture)

pytestmark = pytest.mark.gpu

# launch paths: (name, environment); every Tokenizer is made after its environment is set
PATHS = [
    ("default", {}),
    ("window", {"KGPU_POOL": "0"}),
    ("general", {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}),
    ("team", {"KGPU_WINDOW_TEAM": "2", "KGPU_WINDOW_FIRST": "0"}),
]
KNOBS = CHAIN_KNOBS + ("KGPU_NO_SMALL_CALLS",)


def _same(tok, orc, sentences, what):
    host_batch(tok, orc, sentences, 16, what)


def _tok(d, env, monkeypatch):
    from kanpyo_amd import Tokenizer

    set_env(monkeypatch, env, KNOBS)
    return Tokenizer(d)


def _small_call(sents):
    """At most 128 sentences and 16 KB: the single-launch path (kgpu_small.cpp)."""
    out, size = [], 0
    for s in sents:
        b = len(s.encode())
        if len(out) == 128 or size + b > 16384:
            break
        out.append(s); size += b
    return out


def _compact_vs_full(tok, orc, sents):
    """kgpu_tokenize_device_compact (8-byte records, expanded on the host) against kgpu_tokenize_device (24-byte) and the oracle."""
    import torch

    from kanpyo_amd.device import DeviceContext, expand_tokens
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sents)
    exp = orc.tokenize_batch(utf8, offs, 16)
    dev = torch.device("cuda", 0)
    n, cap = len(sents), int(offs[-1]) + len(sents)
    d_utf8 = torch.from_numpy(utf8.copy()).to(dev) if utf8.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_t8, d_first = torch.empty((cap, 2), dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
    d_toff, d_st = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.full((n,), STATUS_MARKER, dtype=torch.uint8, device=dev)
    ctx = DeviceContext(tok)
    ctx.tokenize_compact(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_t8.data_ptr(), cap, d_first.data_ptr(), d_toff.data_ptr(), d_st.data_ptr())
    nt = ctx.sync()
    nt24, _ = device_batch(ctx, orc, sents, exp, what="24-byte records")
    ctx.close()
    toff = d_toff.cpu().numpy().astype(np.uint64)
    assert nt == nt24 == len(exp.tokens), (nt, nt24, len(exp.tokens))
    assert np.array_equal(toff, exp.offsets), "8-byte records: per-sentence token counts differ"
    assert_records(d_st.cpu().numpy(), toff, expand_tokens(d_t8[:nt].cpu().numpy(), toff, d_first.cpu().numpy()), exp, sents, "8-byte records")


def _every_path(d, sents, what, monkeypatch, oracle):
    orc = oracle.OracleTokenizer.from_dict(d)
    for name, env in PATHS:
        tok = _tok(d, env, monkeypatch)
        _same(tok, orc, sents, f"{what} path={name}")
        tok.close()
    tok = _tok(d, {}, monkeypatch)
    small = _small_call(sents)
    _same(tok, orc, small, f"{what} small call")
    monkeypatch.setenv("KGPU_NO_SMALL_CALLS", "1")
    _same(tok, orc, small, f"{what} small call, KGPU_NO_SMALL_CALLS")
    monkeypatch.delenv("KGPU_NO_SMALL_CALLS")
    _compact_vs_full(tok, orc, sents)
    return tok


@pytest.mark.parametrize("shape", ["square", "nonsquare", "flat", "corner", "big_rows", "huge"])
def test_matrix_shapes_every_path(libs, shape, monkeypatch):
    """One dictionary of the shape per cost mode (plain, i16 extremes, ties), each under every launch path, the small-call
    path with and without KGPU_NO_SMALL_CALLS, and the 8-byte device API; info() reports the shape as given."""
    from kanpyo_amd import synth

    _, oracle = libs
    for k, cost in enumerate(synth.MATRIX_COSTS):
        rng = random.Random(1000 * k + len(shape))
        d, sents, meta = synth.matrix_case(rng, shape, cost)
        assert meta["shape"] == shape and meta["cost"] == cost
        sents = sents[:800] + ["", "x", "ああ" * 40, "あいあいか" * 700]
        tok = _every_path(d, sents, f"{meta}", monkeypatch, oracle)
        info = tok.info()
        assert (info["conn_rows"], info["conn_cols"]) == (meta["rows"], meta["cols"])


def test_hand_dictionaries_every_path(libs, monkeypatch):
    """tests/test_matrix_cpu.py's 3x2 dictionary, where reading the matrix by cols would change the token."""
    from kanpyo_amd import Dict

    _, oracle = libs
    d = Dict.from_parts(**transposed_parts())
    sents = ["あい", "あいあい", "あ", "いあ", "", "あいう" * 1200] + ["".join(random.Random(k).choices("あいx", k=k % 300 + 1)) for k in range(300)]
    _every_path(d, sents, "3x2 hand dictionary", monkeypatch, oracle)


def test_saturation_and_truncated_backtrace_across_windows(libs, monkeypatch):
    """dp driven to INF by accumulation: 50 KB sentences whose backtrace stops in the middle of a multi-window document
    (tests/test_matrix_cpu.py derives the answers by hand), on the windowed, general and team paths; and the 3x3 dead-end
    dictionary of test_unreachable_eos_and_dead_ends with its sentences repeated past 3072 bytes."""
    from kanpyo_amd import Dict
    from kanpyo_amd.tokenizer import pack_sentences

    _, oracle = libs
    d = Dict.from_parts(**saturation_parts())
    orc = oracle.OracleTokenizer.from_dict(d)
    sents = ["あ" * n + "い" * m for n in (16383, 16384, 16385, 16386, 17000) for m in (0, 3, 5)]
    exp = orc.tokenize_batch(*pack_sentences(sents), 16)
    assert [int(exp.offsets[i + 1] - exp.offsets[i]) for i in range(len(sents))][-3:] == [0, 4, 6]   # the hand answers of 17000
    for name, env in PATHS:
        tok = _tok(d, env, monkeypatch)
        _same(tok, orc, sents, f"saturation path={name}")
        tok.close()
    p = fixture_dict_parts()
    p["conn_data"] = [0, 100, 200, 100, -30000, 100, 200, 100, -30000]
    p["morphs"] = [[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]]
    d = Dict.from_parts(**p)
    orc = oracle.OracleTokenizer.from_dict(d)
    base = ["テ", "テあ", "テ辞書", "テ辞書形態素", "テスト辞書", "ト辞書あ", "辞書テ", "形態素テ形態素", "テテ辞書辞書"]
    sents = [s * (3100 // len(s.encode()) + 1) for s in base] + base
    for name, env in PATHS:
        tok = _tok(d, env, monkeypatch)
        _same(tok, orc, sents, f"dead ends path={name}")
        tok.close()


def _uniform_cost_dict(value, dups, seed):
    """Surfaces of one to three characters over あいう, `dups` records each, every word, unknown word and matrix cost
    equal to `value`, on a 4x6 matrix with ids spread over it."""
    from kanpyo_amd import Dict

    nr = np.random.default_rng(seed)
    words = sorted({"".join(w) for n in (1, 2, 3) for w in itertools.product("あいう", repeat=n)}, key=lambda s: s.encode())
    recs = [w for w in words for _ in range(int(nr.integers(1, dups + 1)))]
    morphs = np.stack([nr.integers(0, 6, len(recs)), nr.integers(0, 4, len(recs)), np.full(len(recs), value)], axis=1)
    cat = np.zeros(65536, dtype=np.uint8)
    for ch in "あいう":
        cat[ord(ch)] = 1
    return Dict.from_parts(recs, morphs, 4, 6, np.full(24, value), ["DEFAULT", "H"], cat, np.array([0, 1], dtype=np.uint8),
                           np.array([1, 1], dtype=np.uint8), {0: (1, 1), 1: (2, 2)}, [(0, 0, value), (5, 3, value), (2, 1, value)])


def test_negative_drift(libs, monkeypatch):
    """Every cost -32768: dp falls by up to 65 536 a character, to about -1.05e9 on 16 000 characters (still above
    -2^31), through every 16-bit cost field and every i32 sum of the kernels."""
    _, oracle = libs
    d = _uniform_cost_dict(-32768, 2, 7)
    rng = random.Random(7)
    sents = ["".join(rng.choices("あいうx", k=n)) for n in (1, 2, 50, 500, 3000, 9000, 16000)] + ["あ" * 16000, "う" * 15999 + "x"]
    orc = oracle.OracleTokenizer.from_dict(d)
    for name, env in PATHS:
        tok = _tok(d, env, monkeypatch)
        _same(tok, orc, sents, f"negative drift path={name}")
        tok.close()


def test_ties_everywhere(libs, monkeypatch):
    """Every cost 0: every total ties, and the best predecessor is the first in insertion order (strict '<',
    lattice.rs:125,136) -- across a target's predecessor chunks, windows and the streamed buckets of the windowed kernel."""
    _, oracle = libs
    d = _uniform_cost_dict(0, 40, 8)
    rng = random.Random(8)
    sents = ["".join(rng.choices("あいうx", k=rng.choice([1, 5, 40, 120]))) for _ in range(600)] + ["".join(rng.choices("あいう", k=n)) for n in (1500, 4000)]
    _every_path(d, sents, "ties", monkeypatch, oracle)


def test_lattice_dump_ranked_and_unranked(libs, monkeypatch):
    """kgpu_lattice_dump on a ranked non-square dictionary and on unranked ones (right ids >= rows; an axis of 65 536 or
    more): node for node equal to the naive restatement's lattice, in the dictionary's own ids, and the same DOT."""
    from kanpyo_amd import Dict, Tokenizer, synth
    from kanpyo_amd.lattice import dump_lattice, graphviz
    from oracle import pyref

    cases = [(Dict.from_parts(**transposed_parts()), True)]
    for shape in ("nonsquare", "flat", "huge"):
        d, _, meta = synth.matrix_case(random.Random(77), shape, "plain")
        cases.append((d, meta["ranked"]))
    assert {r for _, r in cases} == {True, False}
    f = lambda i: ["x"]  # noqa: E731
    for d, _ranked in cases:
        tok = _tok(d, {}, monkeypatch)
        pd = pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
        conn = lambda r, l: pd.conn[pd.row * l + r]  # noqa: E731
        for text in ["", "あ", "あい", "いあx", "あいうえおか" * 5, "xあxいx", "ああああいいいいか" * 3]:
            got, exp = dump_lattice(tok, text), lattice_from_pyref(pd, text)
            assert got.edges == exp.edges, text
            assert got.nodes == exp.nodes, text
            for full_state in (False, True):
                assert graphviz(got, conn, f, f, 48, full_state) == graphviz(exp, conn, f, f, 48, full_state)
        tok.close()
    # the saturated lattice: dp = INF and no predecessor on the あ from 16 386 on
    d = Dict.from_parts(**saturation_parts())
    pd = pyref.PyDict(d.index_dict, d.connection_dict, d.morph_dict, d.unk_dict, d.char_category, d.invoke_list, d.group_list)
    tok = Tokenizer(d)
    text = "あ" * 16390 + "いい"
    got, exp = dump_lattice(tok, text), lattice_from_pyref(pd, text)
    assert got.nodes == exp.nodes and got.edges == exp.edges
    assert got.nodes[16386].dp == 1 << 30 and got.nodes[16386].pre is None and got.nodes[16385].pre == 16384
