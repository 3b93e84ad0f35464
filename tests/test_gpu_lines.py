"""The `kanpyo tokenize` output on the device (src/bin/kanpyo.rs:106-126, 174-197): kgpu_tokenize_batch_lines, kgpu_format_lines_device,
the C consumer and `python -m kanpyo_amd tokenize`.  Expected bytes always come from the oracle's tokens (or the hand-derived fixture
tokens) and MorphFeatureTable.features in Python -- never from the library's parser, pool or kernels.  These tests reach the renderer
(kgpu_format.hip) with records the tokenizer wrote; its direct tests on crafted records -- every destination misalignment, window edges, more
than 32 768 sentences, output past 4 GiB, bad records late in the work -- are tests/test_gpu_format.py, against tests/lines_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, fixture_dict_parts, load_golden
from lines_ref import expected_lines
from record_cases import _write_dict_dir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth_full():
    from kanpyo_amd import Tokenizer, synth
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return sd, tok, oracle.OracleTokenizer.from_dict(sd.dict), known, unk


def _check(tok, orc, known, unk, sents):
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sents)
    text, toff, status = tok.tokenize_lines_packed(utf8, offs)
    exp = orc.tokenize_batch(utf8, offs, 8)
    want, want_off = expected_lines(utf8, offs, exp.tokens, exp.offsets, known, unk)
    assert text.tobytes() == want
    assert np.array_equal(toff, want_off)
    return status


def test_cfg2_batch(synth_full):
    from kanpyo_amd import synth

    sd, tok, orc, known, unk = synth_full
    st = _check(tok, orc, known, unk, synth.make_corpus(sd, 4096, 1, "cfg2"))
    assert not st.any()


def test_cfg3_mix_reaches_every_kernel(synth_full):
    from kanpyo_amd import synth

    sd, tok, orc, known, unk = synth_full
    routing0 = tok.routing(reset=True)  # noqa: F841
    sents = synth.make_corpus(sd, 1500, 2, "cfg3") + synth.make_corpus(sd, 4, 5, "cfg5") + ["あ" * 9000]
    _check(tok, orc, known, unk, sents)
    r = tok.routing()
    assert r["deferred"][0] > 0   # sentences left the LDS-resident kernel for the windowed (and further) kernels


@pytest.mark.parametrize("env", [{"KGPU_POOL": "0"}, {"KGPU_POOL": "0", "KGPU_WINDOW": "0"}, {"KGPU_NO_SMALL_CALLS": "1"}])
def test_forced_chains(synth_full, env, monkeypatch):
    from kanpyo_amd import Tokenizer, synth

    sd, _, orc, known, unk = synth_full
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tok = Tokenizer(sd.dict)   # (a fresh handle: the chain is planned per context)
    tok.set_features(known, unk)
    _check(tok, orc, known, unk, synth.make_corpus(sd, 300, 3, "cfg2") + synth.make_corpus(sd, 40, 4, "cfg3"))


def test_many_chunks_and_tiny_calls(synth_full, monkeypatch):
    from kanpyo_amd import synth

    sd, tok, orc, known, unk = synth_full
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "1000")
    _check(tok, orc, known, unk, synth.make_corpus(sd, 9000, 6, "cfg2"))
    monkeypatch.delenv("KGPU_HOST_CHUNK_SENTS")
    _check(tok, orc, known, unk, synth.make_corpus(sd, 30000, 7, "cfg2"))
    _check(tok, orc, known, unk, [])
    _check(tok, orc, known, unk, ["すもももももももものうち"])
    _check(tok, orc, known, unk, [""])


def test_fixture_dictionary_hand_derived():
    """The reference's fixture dictionary (src/tests.rs:8-108) and its hand-derived tokens (tests/golden/fixture_tokens.json)."""
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.dictfile import MorphFeatureTable
    from kanpyo_amd.tokenizer import pack_sentences

    p = fixture_dict_parts()
    d = Dict.from_parts(**p)
    known = MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(p["morphs"]) + 1)])
    unk = MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, len(p["unk_morphs"]) + 1)])
    tok = Tokenizer(d)
    tok.set_features(known, unk)
    cases = load_golden("fixture_tokens.json")["cases"]
    want = b""
    for c in cases:
        for tid, cls, _pos, _start, _end, surface in c["tokens"]:   # (id, class, position, start, end, surface), hand-derived
            feats = "" if cls == 0 or tid == 0 else (f"名詞,k{tid},*" if cls == 1 else f"未知語,u{tid}")
            want += f"{surface}\t{feats}\n".encode()
    utf8, offs = pack_sentences([c["input"] for c in cases])
    text, _, _ = tok.tokenize_lines_packed(utf8, offs)
    assert text.tobytes() == want


def test_edge_cases(synth_full):
    from kanpyo_amd import Dict, Tokenizer, _lib
    from kanpyo_amd.dictfile import MorphFeatureTable
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    sd, tok, orc, known, unk = synth_full
    assert tok.tokenize_lines([""]) == b"EOS\t\n"
    # invalid UTF-8: status 1, no bytes; its neighbours are unaffected
    utf8, offs = pack_sentences([b"\xe3\x81", "あ".encode(), b"\xff"])
    text, toff, st = tok.tokenize_lines_packed(utf8, offs)
    assert st.tolist() == [1, 0, 1] and toff[1] == toff[0] == 0 and toff[3] == toff[2] and text.tobytes().endswith(b"EOS\t\n")
    # a 1024-character unknown run (MAX_UNKNOWN_LEN, lattice.rs:55) and beyond
    _check(tok, orc, known, unk, ["ア" * 1024, "ゞ" * 1030, "x" * 2000])
    # an unreachable EOS renders nothing; empty rows, a 10 KB feature string, id 0 fields
    p = fixture_dict_parts()
    p["conn_data"] = [0, 100, 200, 100, -30000, 100, 200, 100, -30000]
    p["morphs"] = [[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]]
    d = Dict.from_parts(**p)
    k = MorphFeatureTable([[], [1, 0, 1], [2]], ["", "名" * 10, "長" * 3400])
    u = MorphFeatureTable([[1]] * len(p["unk_morphs"]), ["", "未知"])
    t2 = Tokenizer(d)
    t2.set_features(k, u)
    o2 = oracle.OracleTokenizer.from_dict(d)
    sents = ["テ", "テあ", "テ辞書", "テ辞書形態素", "テスト辞書", "ト辞書あ", "辞書テ", "形態素テ形態素", "テテ辞書辞書"]
    utf8, offs = pack_sentences(sents)
    exp = o2.tokenize_batch(utf8, offs, 1)
    assert (np.diff(exp.offsets) == 0).any(), "the case needs a sentence whose EOS is unreachable"
    _check(t2, o2, k, u, sents)
    # KGPU_ERR_CAPACITY reports the exact size
    L = _lib.lib()
    import ctypes as C

    utf8, offs = pack_sentences(["すもももももももものうち", "テスト"])
    want, _, _ = tok.tokenize_lines_packed(utf8, offs)
    buf = np.zeros(len(want), dtype=np.uint8)
    toff = np.zeros(3, dtype=np.uint64)
    got = C.c_uint64(0)
    rc = L.kgpu_tokenize_batch_lines(tok.handle, utf8.ctypes.data, offs.ctypes.data, 2, buf.ctypes.data, len(want) - 1, toff.ctypes.data, None, C.byref(got))
    assert rc == _lib.KGPU_ERR_CAPACITY and got.value == len(want)
    rc = L.kgpu_tokenize_batch_lines(tok.handle, utf8.ctypes.data, offs.ctypes.data, 2, buf.ctypes.data, len(want), toff.ctypes.data, None, C.byref(got))
    assert rc == _lib.KGPU_OK and buf.tobytes() == want.tobytes()


def test_device_form_matches_the_host_form(synth_full):
    import torch

    from kanpyo_amd import synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, orc, known, unk = synth_full
    utf8, offs = pack_sentences(synth.make_corpus(sd, 4096, 8, "cfg2") + synth.make_corpus(sd, 50, 9, "cfg3"))
    host, host_off, _ = tok.tokenize_lines_packed(utf8, offs)
    dev = torch.device("cuda", 0)
    n, cap = len(offs) - 1, int(offs[-1]) + len(offs)
    d_utf8 = torch.from_numpy(utf8.copy()).to(dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx = DeviceContext(tok)
    ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
    ctx.sync()
    for shift in (0, 3):   # an unaligned destination: head and tail units of the buffer
        d_text = torch.full((len(host) + 64,), 0xAB, dtype=torch.uint8, device=dev)
        d_text_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ctx.format_lines(d_utf8.data_ptr(), d_off.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_text.data_ptr() + shift, len(host), d_text_off.data_ptr())
        assert ctx.sync_lines() == len(host)
        t = d_text.cpu().numpy()
        assert t[shift : shift + len(host)].tobytes() == host.tobytes()
        assert (t[:shift] == 0xAB).all() and (t[shift + len(host) :] == 0xAB).all()
        assert np.array_equal(d_text_off.cpu().numpy().astype(np.uint64), host_off)
    # too small: nothing written, the size reported
    d_text = torch.full((len(host),), 0xAB, dtype=torch.uint8, device=dev)
    ctx.format_lines(d_utf8.data_ptr(), d_off.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_text.data_ptr(), len(host) - 1, d_text_off.data_ptr())
    from kanpyo_amd import _lib

    with pytest.raises(_lib.KgpuError) as e:
        ctx.sync_lines()
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and (d_text.cpu().numpy() == 0xAB).all()
    ctx.close()


def test_set_features_errors(synth_full):
    from kanpyo_amd import Tokenizer, _lib
    from kanpyo_amd.dictfile import MorphFeatureTable

    sd, tok, orc, known, unk = synth_full
    t = Tokenizer(sd.dict)
    with pytest.raises(_lib.KgpuError) as e:
        t.tokenize_lines(["あ"])
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "kgpu_dict_set_features" in str(e.value)
    with pytest.raises(_lib.KgpuError) as e:
        t.set_features(MorphFeatureTable(known.morph_features[:-1], known.name_list), unk)
    assert e.value.code == _lib.KGPU_ERR_BAD_DICT
    with pytest.raises(_lib.KgpuError) as e:
        t.set_features(known, MorphFeatureTable(unk.morph_features[:-1], unk.name_list))
    assert e.value.code == _lib.KGPU_ERR_BAD_DICT
    b0 = t.info()["device_bytes"]
    t.set_features(known, unk)
    assert t.info()["device_bytes"] > b0
    with pytest.raises(_lib.KgpuError) as e:
        t.set_features(known, unk)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    assert t.tokenize_lines([""]) == b"EOS\t\n"


def _stdin_case(sd, orc, known, unk):
    """An input file with CRLF and U+3000-trailing lines, a blank line and no final newline -> (bytes, expected stdout)."""
    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import pack_sentences

    sents = synth.make_corpus(sd, 3000, 11, "cfg2")
    raw = []
    for i, s in enumerate(sents):
        tail = ["\r\n", "　\n", " \t\n", "\n"][i % 4]
        raw.append(s + tail)
    raw.insert(5, "\n")
    data = "".join(raw).encode() + "最後の行".encode()
    # read_line + trim_end restated (the corpus has spaces and control characters of its own, '\n' among them)
    ws = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(map(chr, range(0x2000, 0x200B))) + "\u2028\u2029\u202f\u205f\u3000"
    lines = [ln.rstrip(ws) for ln in data.decode().split("\n")]
    utf8, offs = pack_sentences(lines)
    exp = orc.tokenize_batch(utf8, offs, 8)
    return data, expected_lines(utf8, offs, exp.tokens, exp.offsets, known, unk)[0]


def test_c_consumer_matches(synth_full, tmp_path):
    from kanpyo_amd import _lib
    from kanpyo_amd.dictfile import DictFile

    sd, tok, orc, known, unk = synth_full
    exe = str(tmp_path / "lines_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "lines_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    blobs = _write_dict_dir(sd.dict, DictFile(sd.dict, known, unk), tmp_path)
    data, want = _stdin_case(sd, orc, known, unk)
    r = subprocess.run([exe, str(blobs)], input=data, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want


def test_cli_stdout_is_the_reference_output(synth_full, tmp_path):
    from kanpyo_amd.dictfile import DictFile, save_dict

    sd, tok, orc, known, unk = synth_full
    path = tmp_path / "t.dict"
    save_dict(DictFile(sd.dict, known, unk), str(path))
    data, want = _stdin_case(sd, orc, known, unk)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)]
    r = subprocess.run(cmd + ["--block-bytes", "20000"], input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    # an invalid line: the lines before it, then a panic's exit status
    cut = data.index(b"\n", len(data) // 2) + 1
    r = subprocess.run(cmd + ["--block-bytes", "20000"], input=data[:cut] + b"\xff\xfe\n" + data[cut:], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 101
    n_before = data[:cut].count(b"\n")
    assert r.stdout == want[: _offset_of_line(want, n_before)]
    # INPUT argument: that one string, untrimmed
    r = subprocess.run(cmd + ["すもも "], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.endswith(b"EOS\t\n") and r.stdout.count(b"EOS\t\n") == 1


def _offset_of_line(text: bytes, k: int) -> int:
    """Byte offset where sentence k's lines start (every sentence ends with its EOS line)."""
    at = 0
    for _ in range(k):
        at = text.index(b"EOS\t\n", at) + 5
    return at


# ---- the two branches of a lines chunk's finish, through both host entry points -------------------------------------------------------------
def _lines_call(tok, entry, block, text_capacity=None):
    """The block's lines through one host entry point -> (text, text_offsets, status).  text_capacity: the C call itself with a text buffer
    of that size (so that a first call on fresh contexts is the one that delivers), else the Python wrapper."""
    import ctypes as C

    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import split_lines

    if entry == "packed":
        utf8, offs = split_lines(block)
        if text_capacity is None:
            return tok.tokenize_lines_packed(utf8, offs)
        n = len(offs) - 1
        return tok.tokenize_lines_packed(utf8, offs, out=(np.empty(text_capacity, dtype=np.uint8), np.empty(n + 1, dtype=np.uint64), np.empty(max(n, 1), dtype=np.uint8)))
    if text_capacity is None:
        return tok.tokenize_text_lines(block)
    src = np.frombuffer(block, dtype=np.uint8)
    ocap = block.count(b"\n") + 2
    text, toff, status = np.empty(text_capacity, dtype=np.uint8), np.empty(ocap, dtype=np.uint64), np.zeros(ocap, dtype=np.uint8)
    n, got = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().kgpu_tokenize_text_lines(tok.handle, src.ctypes.data, src.size, text.ctypes.data, text_capacity, toff.ctypes.data, ocap,
                                                   status.ctypes.data, C.byref(n), C.byref(got)))
    return text[: got.value], toff[: n.value + 1], status[: n.value]


def _oracle_lines(orc, known, unk, block):
    from kanpyo_amd.tokenizer import split_lines

    utf8, offs = split_lines(block)
    exp = orc.tokenize_batch(utf8, offs, 8)
    return expected_lines(utf8, offs, exp.tokens, exp.offsets, known, unk)


@pytest.mark.parametrize("entry", ["packed", "text"])
def test_chain_runs_again_behind_the_render(entry):
    """A chunk whose chain ended without its tail and needed it runs the tail inside kgpu_ctx_sync, behind the render that was queued with the first
    pass: the chunk's finish renders once more, and the bytes are the oracle's.  The recipe of test_gpu_parity.py::
    test_chain_tail_is_left_out_and_comes_back: clean short batches disarm the tail (the arming is the dictionary's), then a mixed batch."""
    from kanpyo_amd import Tokenizer, synth
    from oracle import oracle

    oracle.build()
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    tok, orc = Tokenizer(sd.dict), oracle.OracleTokenizer.from_dict(sd.dict)
    tok.set_features(known, unk)
    short = [s[:30].replace("\n", "") for s in synth.make_corpus(sd, 600, 9, "cfg2")]
    clean = "".join(s + "\n" for s in short).encode()
    for _ in range(14):
        _lines_call(tok, entry, clean)
    assert tok.routing()["tail_reruns"] == 0
    mixed = short[:100] + ["ア" * 900, "漢字かな" * 150] + [s.replace("\n", "") for s in synth.make_corpus(sd, 5, 10, "cfg3")] + short[100:200]
    block = "".join(s + "\n" for s in mixed).encode()
    want, want_off = _oracle_lines(orc, known, unk, block)
    text, toff, status = _lines_call(tok, entry, block)
    reruns = tok.routing()["tail_reruns"]
    print(f"{entry}: tail_reruns {reruns}")
    assert reruns >= 1, "the mixed batch did not take the tail pass: the render-again branch was not reached"
    assert not status.any()
    assert np.array_equal(toff, want_off)
    assert text.tobytes() == want


@pytest.mark.parametrize("entry", ["packed", "text"])
def test_chunk_text_outgrows_the_first_block(entry):
    """A chunk's mapped text block is sized by a guess and grown to the size the render reports; the render then runs again.  On the small dictionary
    of test_edge_cases, whose third morph carries a feature string of 10 200 bytes, a chunk of at most 48 input bytes gets a first block of
    48 * 16 + 4096 = 4864 bytes (LinesChunk::prepare), which PinBuf::ensure rounds up by a quarter plus 4096: 4864 + 1216 + 4096 = 10 176 bytes --
    one line of that morph alone (surface + tab + 10 200 + newline) is longer, so the grow-and-render-again branch is taken by arithmetic."""
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.dictfile import MorphFeatureTable
    from kanpyo_amd.tokenizer import pack_sentences
    from oracle import oracle

    oracle.build()
    p = fixture_dict_parts()
    p["conn_data"] = [0, 100, 200, 100, -30000, 100, 200, 100, -30000]
    p["morphs"] = [[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]]
    d = Dict.from_parts(**p)
    k = MorphFeatureTable([[], [1, 0, 1], [2]], ["", "名" * 10, "長" * 3400])
    u = MorphFeatureTable([[1]] * len(p["unk_morphs"]), ["", "未知"])
    assert len(",".join(k.features(3)).encode()) == 10200
    orc = oracle.OracleTokenizer.from_dict(d)
    candidates = ["テスト", "辞書", "形態素", "辞書形態素", "形態素テスト", "あ形態素", "テ辞書形態素", "形態素形態素", "テスト辞書"]
    utf8, offs = pack_sentences(candidates)
    exp = orc.tokenize_batch(utf8, offs, 1)
    with_third = [s for i, s in enumerate(candidates)
                  if any(int(t["cls"]) == 1 and int(t["id"]) == 3 for t in exp.tokens[int(exp.offsets[i]) : int(exp.offsets[i + 1])])]
    lines, total = [], 0
    for s in sorted(with_third, key=lambda s: len(s.encode())):   # a few of them, 48 input bytes at most
        if len(lines) < 3 and total + len(s.encode()) <= 48:
            lines.append(s)
            total += len(s.encode())
    assert lines, "no candidate's oracle tokens include the third morph"
    need = total * 16 + 4096
    first_block = need + need // 4 + 4096
    assert first_block < 10200
    block = "".join(s + "\n" for s in lines).encode()
    want, want_off = _oracle_lines(orc, k, u, block)
    print(f"{entry}: {len(lines)} lines, {total} input bytes, first block {first_block}, rendered {len(want)}")
    assert len(want) > first_block
    tok = Tokenizer(d)   # (fresh contexts: their text blocks start at the first guess)
    tok.set_features(k, u)
    text, toff, status = _lines_call(tok, entry, block, text_capacity=len(want) + 64)   # delivered by the call that grew the block
    assert not status.any()
    assert np.array_equal(toff, want_off)
    assert text.tobytes() == want
    text, toff, status = _lines_call(tok, entry, block)   # ... and through the wrapper, whose own first buffer is too small as well
    assert np.array_equal(toff, want_off) and text.tobytes() == want
