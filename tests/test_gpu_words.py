"""The wakati output on the device (include/kanpyo_gpu.h, "wakati-gaki"; kgpu_words.hip): kgpu_tokenize_batch_words,
kgpu_tokenize_text_words, kgpu_format_words_device, the C consumer and `python -m kanpyo_amd wakati`.  Expected bytes always come from the
oracle's tokens (or crafted records) through tests/words_ref.py -- never from the library's parser, word table or kernels.  No tolerance:
text and all n + 1 text offsets are compared byte for byte."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lines_ref as R
import words_ref as W
from conftest import ROOT, fixture_dict_parts, load_golden
from record_cases import FILL, POS_DROP, SPECS, _Dest, _Env, _Input, _sync, _write_dict_dir, ref_spec, small_env  # noqa: F401  (small_env: the fixture)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def full():
    from kanpyo_amd import synth

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    e.sd = sd
    return e


def _mix(sd):
    from kanpyo_amd import synth

    return synth.make_corpus(sd, 1500, 2, "cfg3") + synth.make_corpus(sd, 4, 5, "cfg5") + ["あ" * 9000]


# ---- full-size dictionary ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPECS))
def test_cfg2_batch(full, name):
    from kanpyo_amd import synth

    sents = synth.make_corpus(full.sd, 4096, 1, "cfg2")
    counts = {}
    text, toff, status, _ = full.check(sents, SPECS[name], counts)
    assert not status.any() and len(toff) == 4097 and text.tobytes().count(b"\n") >= 4096
    sizes = np.diff(toff.astype(np.int64))
    print(f"{name}: {counts['tokens']} tokens, {counts['dropped']} dropped, {int((sizes == 1).sum())} empty lines, {len(text)} bytes")
    if name == "drop":
        assert 0 < counts["dropped"] < counts["tokens"], "the DROP filter must drop some tokens and keep some"
    if name == "keep":
        assert (sizes == 1).any() and (sizes > 1).any(), "KEEP [感動詞] must give both empty and non-empty lines"
    if name not in ("drop", "keep"):
        assert counts["dropped"] == 0


@pytest.mark.parametrize("name", list(SPECS))
def test_cfg3_mix_reaches_every_kernel(full, name):
    full.tok.routing(reset=True)
    counts = {}
    text, toff, _, _ = full.check(_mix(full.sd), SPECS[name], counts)
    assert full.tok.routing()["deferred"][0] > 0   # sentences left the LDS-resident kernel for the windowed (and further) kernels
    sizes = np.diff(toff.astype(np.int64))
    if name == "drop":
        assert 0 < counts["dropped"] < counts["tokens"]
    if name == "keep":
        assert (sizes == 1).any() and (sizes > 1).any()


def test_field6_differs_from_every_surface():
    """synth.feature_tables makes field 6 the surface itself: a table whose column 6 is no surface shows that field 6 is read at all."""
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import MorphFeatureTable

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    rows = []
    for i in range(len(known.morph_features)):
        f = known.features(i + 1)
        f[6] = f"<{i + 1}>" + f[6][::-1]
        rows.append(f)
    known6 = MorphFeatureTable.from_features(rows)
    surfaces = set(synth.record_surfaces(sd))
    assert not any(r[6] in surfaces for r in rows)
    e = _Env(sd.dict, known6, unk)
    sents = synth.make_corpus(sd, 2000, 3, "cfg2") + synth.make_corpus(sd, 200, 4, "cfg3")
    text6, _, _, _ = e.check(sents, {"field": 6})
    text, _, _, _ = e.check(sents, {})
    assert text6.tobytes() != text.tobytes() and b"<" in text6.tobytes()
    e.check(sents, {"field": 6, "drop": POS_DROP, "separator": "\t"})


def test_drop_counts_of_the_issue():
    """2200 sentences (cfg 2 and cfg 3 mixed) of a 20 000-record dictionary: the DROP filter drops some tokens, keeps some, leaves no line empty."""
    from kanpyo_amd import synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    sents = synth.make_corpus(sd, 2000, 3, "cfg2") + synth.make_corpus(sd, 200, 4, "cfg3")
    counts = {}
    text, toff, _, _ = e.check(sents, SPECS["drop"], counts)
    print(f"dropped {counts['dropped']} of {counts['tokens']}, {len(text)} output bytes")
    assert 0 < counts["dropped"] < counts["tokens"]
    assert (np.diff(toff.astype(np.int64)) > 1).all()


# ---- both other host forms -----------------------------------------------------------------------------------------------------------------
def test_text_form_matches_split_plus_batch(full):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import split_lines

    sents = synth.make_corpus(full.sd, 3000, 11, "cfg2")
    raw = [s + ["\r\n", "　\n", " \t\n", "\n"][i % 4] for i, s in enumerate(sents)]
    raw.insert(5, "\n")
    block = "".join(raw).encode() + "最後の行".encode()
    for name in ("surface", "field7", "drop"):
        w = full.words(**SPECS[name])
        utf8, offs = split_lines(block)
        a = w.render_packed(utf8, offs)
        b = w.render_text(block)
        (want, want_off), _ = full.expect(utf8, offs, SPECS[name])
        assert a[0].tobytes() == want and np.array_equal(a[1], want_off)
        assert b[0].tobytes() == want and np.array_equal(b[1], want_off) and np.array_equal(a[2], b[2])
    assert full.words().render_text(b"")[1].tolist() == [0]


def _device_batch(env, utf8, offs):
    """The batch tokenized on a context: device tensors of the input and the records, the context."""
    import torch

    from kanpyo_amd.device import DeviceContext

    dev = torch.device("cuda", 0)
    n, cap = len(offs) - 1, int(offs[-1]) + len(offs)
    t = {"utf8": torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev), "off": torch.from_numpy(offs.astype(np.int64)).to(dev),
         "tok": torch.empty((cap, 6), dtype=torch.int32, device=dev), "toff": torch.empty(n + 1, dtype=torch.int64, device=dev),
         "st": torch.empty(max(n, 1), dtype=torch.uint8, device=dev)}
    ctx = DeviceContext(env.tok)
    ctx.tokenize(t["utf8"].data_ptr(), t["off"].data_ptr(), n, int(offs[-1]), t["tok"].data_ptr(), cap, t["toff"].data_ptr(), t["st"].data_ptr())
    ctx.sync()
    return ctx, t, n


def test_device_form_matches_the_host_form(full):
    import torch

    from kanpyo_amd import _lib, synth
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(synth.make_corpus(full.sd, 4096, 8, "cfg2") + synth.make_corpus(full.sd, 50, 9, "cfg3"))
    ctx, t, n = _device_batch(full, utf8, offs)
    dev = t["utf8"].device
    for name in ("surface", "field7", "drop", "keep"):
        w = full.words(**SPECS[name])
        host, host_off, _ = w.render_packed(utf8, offs)
        (want, _), _ = full.expect(utf8, offs, SPECS[name])
        assert host.tobytes() == want
        for shift in range(16) if name in ("surface", "drop") else (0, 7):
            d_text = torch.full((64 + len(host) + 64,), 0xAB, dtype=torch.uint8, device=dev)
            d_text_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            assert d_text.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            ctx.format_words(w, t["utf8"].data_ptr(), t["off"].data_ptr(), n, t["tok"].data_ptr(), t["toff"].data_ptr(), d_text.data_ptr() + 64 + shift, len(host),
                             d_text_off.data_ptr())
            assert ctx.sync_lines() == len(host)
            got = d_text.cpu().numpy()
            lead = 64 + shift
            assert got[lead : lead + len(host)].tobytes() == host.tobytes(), (name, shift)
            assert (got[:lead] == 0xAB).all() and (got[lead + len(host) :] == 0xAB).all(), (name, shift)
            assert np.array_equal(d_text_off.cpu().numpy().astype(np.uint64), host_off)
        # short by one: nothing written, the exact size reported
        d_text = torch.full((len(host) + 64,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.format_words(w, t["utf8"].data_ptr(), t["off"].data_ptr(), n, t["tok"].data_ptr(), t["toff"].data_ptr(), d_text.data_ptr(), len(host) - 1, d_text_off.data_ptr())
        nb = C.c_uint64(0)
        assert _lib.lib().kgpu_ctx_sync_lines(ctx._h, C.byref(nb)) == _lib.KGPU_ERR_CAPACITY and nb.value == len(host)
        assert (d_text.cpu().numpy() == 0xAB).all()
    # a context of another dictionary
    other = _Env(full.dict, full.known, full.unk)
    with pytest.raises(_lib.KgpuError) as e:
        ctx.format_words(other.words(), t["utf8"].data_ptr(), t["off"].data_ptr(), n, t["tok"].data_ptr(), t["toff"].data_ptr(), d_text.data_ptr(), len(host), d_text_off.data_ptr())
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    ctx.close()


# ---- chains and chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"KGPU_POOL": "0"}, {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}, {"KGPU_NO_SMALL_CALLS": "1"}])
def test_forced_chains(full, env, monkeypatch):
    from kanpyo_amd import synth

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _Env(full.dict, full.known, full.unk)   # (a fresh handle: the chain is planned per context)
    sents = synth.make_corpus(full.sd, 300, 3, "cfg2") + synth.make_corpus(full.sd, 40, 4, "cfg3")
    for name in ("surface", "field7", "drop"):
        e.check(sents, SPECS[name])


def test_many_chunks_and_tiny_calls(full, monkeypatch):
    from kanpyo_amd import synth

    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "1000")
    sents = synth.make_corpus(full.sd, 9000, 6, "cfg2")
    for name in ("surface", "drop", "keep"):
        full.check(sents, SPECS[name])
    monkeypatch.delenv("KGPU_HOST_CHUNK_SENTS")
    sents = synth.make_corpus(full.sd, 30000, 7, "cfg2")
    for name in ("surface", "field8"):
        full.check(sents, SPECS[name])
    for name in SPECS:
        text, toff, status, _ = full.check([], SPECS[name])
        assert len(text) == 0 and toff.tolist() == [0]
        text, toff, status, _ = full.check([""], SPECS[name])
        assert text.tobytes() == b"\n" and toff.tolist() == [0, 1] and status.tolist() == [0]
    assert full.words().render(["すもももももももものうち", ""])[1] == ""


# ---- crafted records through kgpu_format_words_device ----------------------------------------------------------------------------------------
CRAFT_SPECS = [{}, {"field": 1}, {"drop": ("名" * 10,)}, {"keep": ("名" * 10,), "field": 0, "separator": "|"}, {"keep": ("未知",)}, {"drop": ("",)}]


class _Crafted:
    def __init__(self, env):
        from kanpyo_amd.device import DeviceContext

        self.env = env
        self.ctx = DeviceContext(env.tok)   # never tokenizes

    def run(self, case, kw, mis=0, capacity=None, want=None):
        """Render the crafted case -> (rc, bytes reported, destination).  want: (text, offsets) to hold the destination to."""
        inp = _Input(case)
        cap = (len(want[0]) + 32) if capacity is None else capacity
        dest = _Dest(inp.n, cap, mis)
        import torch

        torch.cuda.synchronize()
        self.ctx.format_words(self.env.words(**kw), inp.utf8.data_ptr(), inp.off.data_ptr(), inp.n, inp.tok.data_ptr(), inp.toff.data_ptr(), dest.text_ptr, cap, dest.offs_ptr)
        rc, nb = _sync(self.ctx)
        return rc, nb, dest

    def check(self, case, kw, mis_set=(0,)):
        env = self.env
        want = W.render(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw))
        for mis in mis_set:
            rc, nb, dest = self.run(case, kw, mis, want=want)
            assert (rc, nb) == (0, len(want[0])), (kw, mis, rc, nb, len(want[0]))
            try:
                dest.holds(*want)
            except AssertionError as e:
                raise AssertionError(f"{kw}, mis {mis}, n {len(case[1]) - 1}, {len(case[2])} records: {e}") from None
        return want


@pytest.fixture(scope="module")
def crafted_small(small_env):
    c = _Crafted(small_env)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def crafted_full(full):
    c = _Crafted(full)
    yield c
    c.ctx.close()


@pytest.mark.parametrize("regime", ["two", "cycle", "big"])
def test_window_token_counts_under_all_filters(crafted_small, regime):
    for T in R.WINDOW_TOKENS:
        case = R.window_case(regime, T)
        for kw in CRAFT_SPECS[:4] + ([{"field": 0}] if regime == "big" else []):
            crafted_small.check(case, kw, R.WINDOW_MIS if T in (0, 1, 64, 65, 193) else (0, 9))


def test_random_small_batches_every_alignment(crafted_small):
    rng = np.random.default_rng(2)
    env = crafted_small.env
    for i in range(60):
        case = R.make_records(rng, int(rng.integers(1, 13)), (0, 4), R.KINDS, env.nk, env.nu, known_ids=[1] * 6 + [2] * 6 + [3])
        crafted_small.check(case, CRAFT_SPECS[i % len(CRAFT_SPECS)], range(16))
    crafted_small.check(R.pack([], []), {}, range(16))
    crafted_small.check(R.pack([b"abc", b"", b"d"], [[], [], []]), {"field": 1}, range(16))


def test_empty_words_space_surfaces_and_noisy_eos(crafted_small):
    """The crafted records of tests/test_words_cpu.py::test_reference_rules_on_crafted_records through the device: EOS records with any id,
    position and length in front, between and behind; a zero-length surface (two separators meet); a surface that is a space; a token without a row."""
    recs = [(0, R.DUMMY, 999, 77), (1, R.KNOWN, 0, 2), (5, R.DUMMY, 0, 0), (0, R.KNOWN, 2, 1), (1, R.KNOWN, 3, 0), (-7, R.DUMMY, 1, 1), (1, R.UNKNOWN, 3, 2)]
    case = R.pack([b"ab cd", b"", b"ab cd"], [recs, [(0, R.KNOWN, 0, 0), (2, R.KNOWN, 0, 0)], recs[::-1]])
    k0 = "名" * 10
    want = crafted_small.check(case, {}, range(16))
    assert want[0] == b"ab    cd\n \ncd    ab\n"
    want = crafted_small.check(case, {"separator": "/"}, range(16))
    assert want[0] == b"ab/ //cd\n/\ncd// /ab\n"
    assert crafted_small.check(case, {"keep": ("未知",)}, range(16))[0] == b"cd\n\ncd\n"      # id 0 matches no name: KEEP drops it
    assert crafted_small.check(case, {"drop": ("未知",)}, range(16))[0] == b"ab   \n \n   ab\n"  # ... and DROP keeps it
    assert crafted_small.check(case, {"keep": (k0,)}, range(16))[0] == b"\n\n\n"             # known id 1 has an empty row, id 2 the name: its surface is empty
    crafted_small.check(case, {"field": 0, "separator": "|"}, range(16))


def _gap_case(pattern, text=b"0123456789abcdef"):
    """One sentence; pattern: per record True = the known id 2 (feature 0 "名名..." , kept by KEEP [that name]), False = the unknown id 1 (dropped)."""
    recs = [((2, R.KNOWN, i % 13, 1 + i % 3) if keep else (1, R.UNKNOWN, i % 11, 2)) for i, keep in enumerate(pattern)]
    return R.pack([text], [recs])


def test_windows_where_nothing_is_kept(crafted_small):
    """Windows of 64 records where nothing is kept between windows where something is; a sentence whose only kept token is its first or its last."""
    keep = {"keep": ("名" * 10,)}
    drop = {"drop": ("未知",), "field": 1}
    T = 64 * 6 + 7
    patterns = {
        "gap2": [w in (0, 3, 6) for w in np.arange(T) // 64],
        "only_first": [i == 0 for i in range(T)],
        "only_last": [i == T - 1 for i in range(T)],
        "last_of_each_window": [i % 64 == 63 for i in range(T)],
        "first_of_window_3": [i == 192 for i in range(T)],
        "none": [False] * T,
        "alternate": [i % 2 == 0 for i in range(T)],
    }
    for name, pat in patterns.items():
        case = _gap_case(pat)
        for kw in (keep, drop):
            want = crafted_small.check(case, kw, R.WINDOW_MIS)
            if name == "none":
                assert want[0] == b"\n"
            if name in ("only_first", "only_last", "first_of_window_3"):
                assert want[0].count(kw.get("separator", " ").encode()) == 0 and len(want[0]) > 1
    # several sentences side by side, empty ones between
    utf8, offsets, tokens, tok_offsets = _gap_case(patterns["gap2"])
    many = R.pack([b"0123456789abcdef"] * 5, [[tuple(int(x) for x in (t["id"], t["cls"], t["position"], t["byte_len"])) for t in tokens[: k * 97]] for k in (4, 0, 1, 0, 3)])
    crafted_small.check(many, keep, (0, 5))


@pytest.mark.parametrize("n", R.MANY_N)
def test_many_sentences(crafted_full, n):
    rng = np.random.default_rng(n)
    env = crafted_full.env
    case = R.many_case(rng, n, env.nk, env.nu, long_at=(0, 32768, 70000) if n == 70001 else ())
    for kw in (SPECS["field7"], SPECS["drop"]):
        crafted_full.check(case, kw, (0, 5))


@pytest.mark.parametrize("place", ["early", "late"])
def test_one_bad_record(crafted_full, place):
    from kanpyo_amd import _lib

    env = crafted_full.env
    rng = np.random.default_rng(7)
    case = R.many_case(rng, 70001, env.nk, env.nu, long_at=(3, 40000))
    s, k = (3, 1) if place == "early" else (40000, 150)
    utf8, offsets, tokens, tok_offsets = case
    B = int(offsets[s + 1] - offsets[s])
    r = int(tok_offsets[s]) + k
    good = tokens[r].copy()
    want = W.render(*case, env.known, env.unk, env.nk, env.nu, ref_spec())
    for field, value in (("id", env.nk + 1), ("id", -1), ("cls", 3), ("position", B + 1), ("byte_len", B + 1)):
        bad = tokens.copy()
        bad[r] = (1, R.KNOWN, 0, 0, 0, 0)
        bad[r][field] = value
        with pytest.raises(ValueError):
            W.render(utf8, offsets, bad, tok_offsets, env.known, env.unk, env.nk, env.nu, ref_spec())
        rc, _, dest = crafted_full.run((utf8, offsets, bad, tok_offsets), {}, 3, want=want)
        assert rc == _lib.KGPU_ERR_INVALID_ARG, (field, value)
        assert dest.margins_intact()
    assert np.array_equal(tokens[r], good)
    crafted_full.check(case, {}, (3,))   # the same context renders the reference bytes afterwards


def test_token_offsets_that_run_backwards(crafted_small):
    from kanpyo_amd import _lib

    case = R.make_records(np.random.default_rng(3), 40, 3, ("known", "unk"), crafted_small.env.nk, crafted_small.env.nu)
    utf8, offsets, tokens, tok_offsets = case
    back = tok_offsets.copy()
    back[20] = back[19] - 2
    with pytest.raises(ValueError):
        W.render(utf8, offsets, tokens, back, crafted_small.env.known, crafted_small.env.unk, crafted_small.env.nk, crafted_small.env.nu, ref_spec())
    rc, _, dest = crafted_small.run((utf8, offsets, tokens, back), {}, 0, capacity=4096)
    assert rc == _lib.KGPU_ERR_INVALID_ARG and dest.margins_intact()
    crafted_small.check(case, {})


# ---- status and capacity -------------------------------------------------------------------------------------------------------------------
def test_invalid_utf8_neighbours(full):
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences([b"\xe3\x81", "あ".encode(), b"\xff"])
    for name in SPECS:
        text, toff, st = full.words(**SPECS[name]).render_packed(utf8, offs)
        assert st.tolist() == [1, 0, 1], name
        (want, want_off), _ = full.expect(utf8[2:5], np.array([0, 3], dtype=np.uint64), SPECS[name])
        assert text.tobytes() == b"\n" + want + b"\n" and toff.tolist() == [0, 1, 1 + len(want), 2 + len(want)]


def test_unreachable_eos_and_odd_rows(small_env):
    from kanpyo_amd.tokenizer import pack_sentences

    sents = ["テ", "テあ", "テ辞書", "テ辞書形態素", "テスト辞書", "ト辞書あ", "辞書テ", "形態素テ形態素", "テテ辞書辞書", ""]
    utf8, offs = pack_sentences(sents)
    exp = small_env.orc.tokenize_batch(utf8, offs, 1)
    assert (np.diff(exp.offsets) == 0).any(), "the case needs a sentence whose EOS is unreachable"
    for kw in CRAFT_SPECS + [{"field": 0}, {"field": 2}]:
        text, toff, status, _ = small_env.check(sents, kw)
        assert (np.diff(toff.astype(np.int64)) >= 1).all() and not status.any()
    # the 10 200-byte name as the word: the chunk's first text block is outgrown and grown
    text, _, _, _ = small_env.check(["形態素形態素", "テスト辞書"] * 3, {"field": 0})
    assert ("長" * 3400).encode() in text.tobytes()


def test_capacity_exact_and_short_by_one(full):
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import pack_sentences

    L = _lib.lib()
    utf8, offs = pack_sentences(["すもももももももものうち", "テスト", ""])
    for name in ("surface", "drop", "keep"):
        w = full.words(**SPECS[name])
        want, want_off, _ = w.render_packed(utf8, offs)
        (ref, _), _ = full.expect(utf8, offs, SPECS[name])
        assert want.tobytes() == ref
        buf = np.full(len(want) + 8, 0xAB, dtype=np.uint8)
        toff = np.zeros(4, dtype=np.uint64)
        got = C.c_uint64(0)
        rc = L.kgpu_tokenize_batch_words(w.handle, utf8.ctypes.data, offs.ctypes.data, 3, buf.ctypes.data, len(want) - 1, toff.ctypes.data, None, C.byref(got))
        assert rc == _lib.KGPU_ERR_CAPACITY and got.value == len(want)
        rc = L.kgpu_tokenize_batch_words(w.handle, utf8.ctypes.data, offs.ctypes.data, 3, buf.ctypes.data, len(want), toff.ctypes.data, None, C.byref(got))
        assert rc == _lib.KGPU_OK and buf[: len(want)].tobytes() == want.tobytes() and (buf[len(want) :] == 0xAB).all() and np.array_equal(toff, want_off)
        # the text form: either capacity may be the one that does not fit
        block = "すもももももももものうち\nテスト\n\n".encode()
        src = np.frombuffer(block, dtype=np.uint8)
        n, st = C.c_uint64(0), np.zeros(4, dtype=np.uint8)
        rc = L.kgpu_tokenize_text_words(w.handle, src.ctypes.data, src.size, buf.ctypes.data, len(want) - 1, toff.ctypes.data, 4, st.ctypes.data, C.byref(n), C.byref(got))
        assert rc == _lib.KGPU_ERR_CAPACITY and (n.value, got.value) == (3, len(want))
        rc = L.kgpu_tokenize_text_words(w.handle, src.ctypes.data, src.size, buf.ctypes.data, len(want), toff.ctypes.data, 3, st.ctypes.data, C.byref(n), C.byref(got))
        assert rc == _lib.KGPU_ERR_CAPACITY and (n.value, got.value) == (3, len(want))
        rc = L.kgpu_tokenize_text_words(w.handle, src.ctypes.data, src.size, buf.ctypes.data, len(want), toff.ctypes.data, 4, st.ctypes.data, C.byref(n), C.byref(got))
        assert rc == _lib.KGPU_OK and buf[: len(want)].tobytes() == want.tobytes() and np.array_equal(toff, want_off)


def test_output_past_4gib(crafted_small):
    """The shape of test_gpu_format.py::test_output_past_4gib with the 10 200-byte name as the word (field 0 of the third known row): 512
    sentences, 460 800 records, pieces of 10 201 bytes: 4 700 620 800 bytes at a destination misaligned by 7, checked on the device -- the
    offsets against the numpy running sum, d_text[:total] as a [T, 10201] matrix whose first 10 200 columns are the name and whose last
    column is the separator, or the newline at each sentence's last record.  Sentences 64..95 hold more than 2^32 bytes together."""
    import torch

    from kanpyo_amd import _lib

    env = crafted_small.env
    counts = np.full(512, 40, dtype=np.int64)
    counts[64:96] = 13800
    case = R.big_case(np.random.default_rng(4), counts)
    T, Wd = int(counts.sum()), 10201
    total = T * Wd
    want_off = np.concatenate([[0], np.cumsum(counts * Wd)]).astype(np.uint64)
    assert total >= 2**32 + 2**28 and ((want_off[:-1] < 2**32) & (want_off[1:] > 2**32)).any() and int((counts[64:96] * Wd).sum()) > 2**32
    inp = _Input(case)
    dest = _Dest(inp.n, total + 32, 7)
    torch.cuda.synchronize()
    crafted_small.ctx.format_words(env.words(field=0, separator="|"), inp.utf8.data_ptr(), inp.off.data_ptr(), inp.n, inp.tok.data_ptr(), inp.toff.data_ptr(),
                                   dest.text_ptr, dest.cap, dest.offs_ptr)
    assert _sync(crafted_small.ctx) == (_lib.KGPU_OK, total)
    assert np.array_equal(dest.offsets(), want_off)
    dev = dest.buf.device
    text = dest.buf[dest.lead : dest.lead + total].view(T, Wd)
    last = np.full(T, ord("|"), dtype=np.uint8)
    last[np.cumsum(counts) - 1] = 10
    assert bool((text[:, Wd - 1] == torch.from_numpy(last).to(dev)).all()), "a piece's trailing byte is not the separator / the sentence's newline"
    name = torch.from_numpy(np.frombuffer(("長" * 3400).encode(), dtype=np.uint8).copy()).to(dev)
    for r0 in range(0, T, 8192):
        ok = (text[r0 : r0 + 8192, : Wd - 1] == name).all(dim=1)
        assert bool(ok.all()), f"piece {r0 + int(torch.nonzero(~ok)[0])} does not hold the name"
    assert dest.margins_intact() and bool((dest.buf[dest.lead + total : dest.lead + dest.cap] == FILL).all())
    del text, dest, inp
    torch.cuda.empty_cache()


# ---- handles, threads, consumers -------------------------------------------------------------------------------------------------------------
def test_two_handles_from_eight_threads(full):
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    specs = [SPECS["field7"], SPECS["drop"]]
    handles = [full.tok.words(**kw) for kw in specs]
    corpora, wants = [], []
    for t in range(8):
        utf8, offs = pack_sentences(synth.make_corpus(full.sd, 700 + 300 * t, 20 + t, "cfg2") + synth.make_corpus(full.sd, 10, 40 + t, "cfg3"))
        corpora.append((utf8, offs))
        wants.append(full.expect(utf8, offs, specs[t % 2])[0])
    errors = []

    def work(t):
        try:
            for _ in range(3):
                text, toff, _ = handles[t % 2].render_packed(*corpora[t])
                if text.tobytes() != wants[t][0] or not np.array_equal(toff, wants[t][1]):
                    errors.append(f"thread {t} differs from the reference")
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for h in handles:
        h.close()


def test_a_handle_outlives_the_dictionary():
    from kanpyo_amd import Tokenizer, _lib, synth
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    with pytest.raises(_lib.KgpuError) as e:
        tok.words()
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "kgpu_dict_set_features" in str(e.value)
    tok.set_features(known, unk)
    info = tok.info()
    w = tok.words(field=7, drop=POS_DROP)
    utf8, offs = pack_sentences(synth.make_corpus(sd, 500, 3, "cfg2"))
    first = w.render_packed(utf8, offs)[0].tobytes()
    tok.close()
    exp = oracle.OracleTokenizer.from_dict(sd.dict).tokenize_batch(utf8, offs, 8)
    want, want_off = W.render(utf8, offs, exp.tokens, exp.offsets, known, unk, info["n_morphs"], info["n_unk_morphs"], ref_spec(field=7, drop=POS_DROP))
    for _ in range(2):
        text, toff, _ = w.render_packed(utf8, offs)
        assert text.tobytes() == want == first and np.array_equal(toff, want_off)
    w.close()


def test_c_consumer_on_the_fixture_golden(tmp_path):
    from kanpyo_amd import Dict, _lib
    from kanpyo_amd.dictfile import DictFile, MorphFeatureTable

    p = fixture_dict_parts()
    d = Dict.from_parts(**p)
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, len(p["unk_morphs"]) + 1)])
    exe = str(tmp_path / "words_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "words_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    blobs = _write_dict_dir(d, DictFile(d, known, unk), tmp_path)
    groups = {}
    for c in load_golden("fixture_words.json")["cases"]:
        groups.setdefault((c["field"], c["filter"], c["separator"], tuple(c["names"])), []).append(c)
    assert len(groups) >= 8
    for (field, filt, sep, names), cases in groups.items():
        data = "".join(c["input"] + "\n" for c in cases).encode()
        r = subprocess.run([exe, str(blobs), str(field), str(filt), str(ord(sep)), *names], input=data, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == "".join(c["line"] for c in cases).encode(), (field, filt, sep, names)
    r = subprocess.run([exe, str(blobs), "-1", "0", "32"], input="テスト\n".encode() + b"\xff\n" + "辞書\n".encode(), capture_output=True, timeout=300)
    assert r.returncode == 101 and r.stdout == "テスト\n".encode()


def test_cli_three_input_forms_and_the_101_exit(tmp_path):
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile, save_dict
    from kanpyo_amd.tokenizer import pack_sentences, split_lines

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    e = _Env(sd.dict, known, unk)
    path = tmp_path / "t.dict"
    save_dict(DictFile(sd.dict, known, unk), str(path))
    sents = synth.make_corpus(sd, 1200, 11, "cfg2")
    raw = [s + ["\r\n", "　\n", " \t\n", "\n"][i % 4] for i, s in enumerate(sents)]
    raw.insert(5, "\n")
    data = "".join(raw).encode() + "最後の行".encode()
    utf8, offs = split_lines(data)
    kw = {"field": 7, "drop": POS_DROP, "separator": "|"}
    (want, want_off), _ = e.expect(utf8, offs, kw)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "wakati", "-c", str(path), "--reading", "--drop", ",".join(POS_DROP), "--separator", "|"]
    for split in ("host", "device"):   # stdin, split on the host and on the device
        r = subprocess.run(cmd + ["--block-bytes", "20000", "--split", split], input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == want, split
    # an invalid line: the lines before it, then status 101
    cut = data.index(b"\n", len(data) // 2) + 1
    r = subprocess.run(cmd + ["--block-bytes", "20000"], input=data[:cut] + b"\xff\xfe\n" + data[cut:], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 101
    assert r.stdout == want[: int(want_off[data[:cut].count(b"\n")])]
    # INPUT argument: that one string, untrimmed
    one = sents[0] + " "
    u1, o1 = pack_sentences([one])
    (want1, _), _ = e.expect(u1, o1, {})
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "wakati", "-c", str(path), one], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout == want1 and r.stdout.count(b"\n") == 1
