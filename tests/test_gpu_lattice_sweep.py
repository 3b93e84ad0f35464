"""The kept lattice, swept: every node the general kernel (k_tokenize_general, kanpyo_amd/csrc/kgpu_kernels.hip) leaves behind against the naive
restatement (oracle/pyref.py), on the crafted catalogue and the seeded sweeps of tests/lattice_cases.py (tests/test_lattice_cases_cpu.py says what
they reach).  The tests of graphviz, N-best, marginals and samples, search / extended mode and the user dictionary compare the device with the host
rule over kgpu_lattice_dump of the same sentence; the host rules are pinned on the CPU over the restatement's lattices.  This file closes the chain:
  a. kgpu_lattice_dump == the restatement's lattice, node for node (id, class, positions, context ids, cost, surface, dp, pre) and edge for edge, with
     the character-level trie (the shipped setting) and with the byte-level one (KGPU_BYTE_TRIE=1);
  b. every batch call that keeps the lattices (keep_lattice: fresh slabs, BOS as a node, a descriptor per sentence) == the host rule over the
     RESTATEMENT's lattice, whole arrays byte for byte, a dictionary's sentences in one call;
  c. the user dictionary the same way, and on the crafted withdrawal cases the decisions themselves.
Integer work, and for the marginals arithmetic that is bit-identical by construction: every comparison is exact."""
import random

import pytest

import lattice_cases as L
from lattice_run import Ref, check_kept, check_user, device_docs
from mode_cases import tie_penalties
from prob_cases import THETAS
from userdict_cases import entries_from

pytestmark = pytest.mark.gpu

SWEEPS = [("random", s) for s in L.RANDOM_SEEDS] + [("dense", s) for s in L.DENSE_SEEDS] + [("width", s) for s in L.WIDTH_SEEDS]
GENERATORS = {"random": L.random_sweep, "dense": L.dense_sweep, "width": L.width_sweep}
INVALID = b"\xe3\x81"


def _tok(d):
    from kanpyo_amd import Tokenizer, _lib

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return Tokenizer(d)


@pytest.fixture(params=["char trie", "byte trie"])
def trie(request, monkeypatch):
    """The two walks of the general kernel: set before the Tokenizer is made."""
    if request.param == "byte trie":
        monkeypatch.setenv("KGPU_BYTE_TRIE", "1")
    else:
        monkeypatch.delenv("KGPU_BYTE_TRIE", raising=False)
    return request.param


@pytest.fixture(scope="module")
def crafted():
    """[(Case, Dict, Ref)] of the catalogue: a sentence's restatement lattice is made once for all tests."""
    out = []
    for case in L.catalogue():
        d = case.make()
        out.append((case, d, Ref(d)))
    return out


@pytest.fixture(scope="module", params=SWEEPS, ids=lambda p: f"{p[0]}-{p[1]}")
def swept(request):
    """[(what, Dict, sentences, Ref)] of one seeded sweep (pytest runs a sweep's tests together: one sweep's lattices live at a time)."""
    name, seed = request.param
    return name, seed, [(what, d, sents, Ref(d)) for what, d, sents in GENERATORS[name](seed)]


def _withdrawal_refs():
    out = []
    for case in L.user_cases():
        d = case.make()
        out.append((case, d, Ref(d)))
    return out


# ---- a. the dump, node for node --------------------------------------------------------------------------------------------------------------------------------
def test_dump_catalogue(crafted, trie):
    n = 0
    for case, d, ref in crafted:
        tok = _tok(d)
        for s in case.sentences:
            ref.assert_dump(tok, s, f"{case.name}, {trie}")
            n += 1
        tok.close()
    for case, d, ref in _withdrawal_refs():
        tok = _tok(d)
        ref.assert_dump(tok, case.sentence, f"{case.name}, {trie}")
        tok.close()
    assert n >= 90


def test_dump_sweep(swept, trie):
    name, seed, dicts = swept
    n = 0
    for what, d, sents, ref in dicts:
        tok = _tok(d)
        for s in sents:
            ref.assert_dump(tok, s, f"{what}, {trie}")
            n += 1
        tok.close()
    assert n >= (2400 if name == "random" else 300)


# ---- b. the kept branch, end to end ------------------------------------------------------------------------------------------------------------------------------
def test_kept_catalogue(crafted):
    rng = random.Random(41)
    for k, (case, d, ref) in enumerate(crafted):
        tok = _tok(d)
        sents = list(case.sentences)
        sents[len(sents) // 2 : len(sents) // 2] = [INVALID, ""]   # one sentence that is not UTF-8 and one empty one between valid ones
        check_kept(tok, ref, sents, THETAS[k % len(THETAS)], tie_penalties(rng), case.name)
        tok.close()


def test_kept_sweep(swept):
    """(graphviz has test_graphviz_sweep: the Python renderer is the slow side of it.)"""
    name, seed, dicts = swept
    rng = random.Random(seed)
    for k, (what, d, sents, ref) in enumerate(dicts):
        tok = _tok(d)
        check_kept(tok, ref, sents, THETAS[k % len(THETAS)], tie_penalties(rng), what, graphviz=False)
        tok.close()


def test_graphviz_sweep(swept):
    name, seed, dicts = swept
    for what, d, sents, ref in dicts:
        tok = _tok(d)
        known, unk = ref.feature_tables()
        tok.set_features(known, unk)
        for full_state in (True, False):
            docs, status = device_docs(tok, sents, 48, full_state)
            assert not status.any(), (what, full_state)
            for s, g, w in zip(sents, docs, ref.graphviz(sents, known, unk, 48, full_state)):
                assert g == w, f"{what}: graphviz(full_state={full_state}) of {s[:40]!r} ({len(s)} characters) differs"
        tok.close()


def test_kept_2049_sentences_span_three_chunks(crafted, monkeypatch):
    """Each family in one call of more than 2048 sentences -- three default chunks of 1024 -- with a sentence that is not UTF-8 and an empty one in
    the middle: the catalogue's short sentences over and over (the parked matches, the sweep step, the characters)."""
    for name in ("KGPU_HOST_GRAPHVIZ_CHUNK_SENTS", "KGPU_HOST_NBEST_CHUNK_SENTS", "KGPU_HOST_PROB_CHUNK_SENTS", "KGPU_HOST_MODE_CHUNK_SENTS", "KGPU_HOST_USER_CHUNK_SENTS"):
        monkeypatch.delenv(name, raising=False)
    rng = random.Random(43)
    for case, d, ref in crafted:
        if case.name not in ("parked matches", "sweep step", "characters, short category table"):
            continue
        short = [s for s in case.sentences if len(s) <= 16]
        sents = [short[(i * 7 + i // 5) % len(short)] for i in range(2049)]
        sents[1030:1030] = [INVALID, ""]
        assert len(sents) == 2051 and len(short) >= 3
        tok = _tok(d)
        assert check_kept(tok, ref, sents, THETAS[0], tie_penalties(rng), f"{case.name} x 2051") >= 14
        entries = entries_from(rng, "".join(short), 6, [-200, 0, 300], nctx=L.contexts_of(d))
        check_user(tok, ref, sents, entries, ("normal", "search"), what=f"{case.name} x 2051")
        tok.close()


# ---- c. the user dictionary ------------------------------------------------------------------------------------------------------------------------------------------
def _spans(got, i, classes) -> set:
    t = got[0][int(got[1][i]) : int(got[1][i + 1])]
    return {(int(r["start"]), int(r["end"])) for r in t if int(r["cls"]) in classes}


def test_user_withdrawal_decisions():
    """The crafted dictionaries: the arrays are the host rule's over the restatement's lattice, and the records show the decision -- the entries are too
    dear to be taken by choice, so a user record stands exactly where the unknown nodes beside it were withdrawn."""
    for case, d, ref in _withdrawal_refs():
        tok = _tok(d)
        s = case.sentence
        sents = [s, INVALID, "", s]
        dear = [e for e in case.entries if e[3] == 30000]
        for entries in (case.entries, dear):
            got = check_user(tok, ref, sents, entries, ("normal", "search"), what=case.name)
        got = got["normal"]   # (the dear entries alone)
        none = check_user(tok, ref, sents, [], ("normal",), what=case.name)["normal"]
        assert got[3].tolist() == [0, 1, 0, 0]
        unknown_starts, user_starts = {a for a, _ in _spans(got, 0, (2,))}, {a for a, _ in _spans(got, 0, (3,))}
        assert not (unknown_starts & case.withdrawn), (case.name, unknown_starts)
        if case.withdrawn:
            assert user_starts and user_starts <= case.withdrawn, (case.name, user_starts)     # the path had to take an entry: what it went around is gone
        else:
            assert not user_starts and got[0].tobytes() == none[0].tobytes(), case.name        # nothing withdrawn: the path of no entries at all
        for q in case.kept_by_invoke:                                                          # kept: the unknown word that covers q is still on the path
            assert any(a <= q < b for a, b in _spans(got, 0, (2,))), (case.name, q)
        assert _spans(got, 3, (2, 3)) == _spans(got, 0, (2, 3))
        tok.close()
    # the twins with the invoke bit of the second flipped: its run loses its unknown words as the first one's does
    d = L.twin_dict((0, 0, 0))
    tok, ref, case = _tok(d), Ref(d), L.user_cases()[2]
    got = check_user(tok, ref, [case.sentence], case.entries, ("normal",), what="twins, neither invokes")["normal"]
    assert {a for a, _ in _spans(got, 0, (3,))} == {0, 3}
    tok.close()


@pytest.mark.parametrize("seed", L.RANDOM_SEEDS)
def test_user_sweep(seed):
    users = 0
    for what, d, sents, entries in L.user_sweep(seed):
        tok = _tok(d)
        got = check_user(tok, Ref(d), sents, entries, ("normal", "search"), what=what)
        users += sum(1 for r in got["normal"][0] if int(r["cls"]) == 3)
        tok.close()
    assert users >= 100, users
