"""Text normalisation on the device (include/kanpyo_gpu.h, "text normalisation"; kgpu_normalize.hip): kgpu_normalize_batch, kgpu_normalize_text,
kgpu_normalize_device, the normalize= keyword of the binding, Vocab.encode_tensor and the CLI.  The expected value is always kgpu_normalize_host (pinned
against unicodedata in tests/test_normalize_cpu.py) and tests/golden/fixture_normalize.json -- never the device's own output.  No tolerance: bytes, all
n + 1 offsets and the status bytes are compared exactly.

The kernel gives every lane one 16-byte unit of the ADDRESS space and every wavefront pass 1024 bytes of it, so where a segment lies relative to those
boundaries depends on the line's address as well as on what stands in front of it in the line: the position test pads with every count from 0 to 70 and
from 1000 to 1040 bytes, which puts the segment across every unit and pass boundary whatever the line's alignment is."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_ref as N
from conftest import ROOT
from kanpyo_amd import _lib
from normalize_cases import DAKUTEN, KA, SENTENCES, env, mixed_lines  # noqa: F401  (env: the fixture)

pytestmark = pytest.mark.gpu


def check_batch(tok, lines, form):
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(lines)
    text, toff, status = tok.normalize_packed(utf8, offs, form)
    want_text, want_off, want_status = N.host_lines(lines, form)
    assert np.array_equal(toff, want_off) and np.array_equal(status, want_status), form
    assert text.tobytes() == want_text.tobytes(), form
    return text, toff, status


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["NFC", "NFKC"])
def test_fixture_parity(env, form):
    _, cases = N.fixture_cases()
    lines = [raw for _, raw, _ in cases]
    text, toff, status = check_batch(env.tok, lines, form)
    raw, o = text.tobytes(), toff.tolist()
    for i, (name, _, exp) in enumerate(cases):
        assert (raw[o[i] : o[i + 1]], int(status[i])) == exp[form], name
    assert 1 in status and 4 in status and 0 in status


# ---- 2. a segment across every unit and pass boundary --------------------------------------------------------------------------------------------------
def test_positions(env):
    pads = list(range(0, 71)) + list(range(1000, 1041))
    lines = []
    for seg in ((KA + DAKUTEN).encode(), "e\u0301".encode(), (KA + DAKUTEN + "Ａ").encode()):
        assert len(seg) in (6, 3, 9)
        lines += [b"p" * pad + seg for pad in pads] + [b"p" * pad + seg + b"q" for pad in pads]
    lines += [b"x" * 1023 + (KA + DAKUTEN).encode(), b"x" * 1024 + (KA + DAKUTEN).encode()]
    for form in ("NFC", "NFKC"):
        text, toff, status = check_batch(env.tok, lines, form)
        assert not status.any()
    raw = text.tobytes()
    assert raw[int(toff[0]) : int(toff[1])] == "ガ".encode() and raw.count("ガ".encode()) == 4 * len(pads) + 2 and raw.count("\u00e9".encode()) == 2 * len(pads)


# ---- 3. nothing composes across lines -----------------------------------------------------------------------------------------------------------------------
def test_line_isolation(env):
    lines = []
    for i in range(40):
        lines += [b"a" * i + KA.encode(), DAKUTEN.encode() + b"b" * i]
    lines += ["e".encode(), "\u0301".encode(), "\u1100".encode(), "\u1161".encode(), "\uac00".encode(), "\u11a8".encode()]
    text, toff, status = check_batch(env.tok, lines, "NFKC")
    raw, o = text.tobytes(), toff.tolist()
    assert raw[o[0] : o[1]] == "カ".encode() and raw[o[1] : o[2]] == "\u3099".encode()   # the mark alone, composed with nothing
    assert "ガ".encode() not in raw and "\u00e9".encode() not in raw and "\uac01".encode() not in raw and not status.any()


# ---- 4. batch shapes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 8200])
def test_batch_shapes(env, n):
    lines = mixed_lines(n, seed=100 + n, max_bytes=200 if n <= 4097 else 40)   # (8200: more lines than the launch has workgroups)
    if n >= 63:
        lines[n // 2] = ("ﾊﾝｶｸｶﾀｶﾅﾃﾞｽ" * 300).encode()[:8192 // 3 * 3]   # one 8 KiB line that is all half-width kana
        lines[7] = b""
        lines[9] = b"\xffbad"
        lines[11] = ("a" + "\u0301" * 65).encode()
    text, toff, status = check_batch(env.tok, lines, "NFKC")
    assert len(toff) == n + 1 and len(status) == n
    if n >= 63:
        assert status[9] == 1 and status[11] == 4 and len(lines[n // 2]) == 8190 and int(toff[n // 2 + 1] - toff[n // 2]) > 7000   # (the voiced pairs shrink)
        check_batch(env.tok, lines, "NFC")


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------------------------------------
def _device_run(ctx, lines, form, capacity):
    """kgpu_normalize_device over torch tensors -> (rc, bytes reported, text buffer with 64 sentinel bytes behind the capacity, offsets, status)."""
    import torch

    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(lines)
    n = len(lines)
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_text = torch.full((capacity + 64,), 0x5A, dtype=torch.uint8, device=dev)
    d_toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), 0x77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.normalize(d_utf8.data_ptr(), d_off.data_ptr(), n, d_text.data_ptr(), capacity, d_toff.data_ptr(), d_st.data_ptr(), form)
    got = C.c_uint64(0)
    rc = _lib.lib().kgpu_ctx_sync_normalize(ctx.handle, C.byref(got))
    return rc, int(got.value), d_text.cpu().numpy(), d_toff.cpu().numpy().view(np.uint64), d_st.cpu().numpy()[:n]


def test_capacity(env):
    from kanpyo_amd.device import DeviceContext

    lines = [("\ufdfa" * 100).encode(), "ｶﾞＡＢＣ".encode(), b"", "東京".encode()]
    want_text, want_off, want_status = N.host_lines(lines, "NFKC")
    exact = int(want_off[-1])
    assert exact > 3300 and int(want_off[1]) == 11 * len(lines[0])   # the 11x line
    ctx = DeviceContext(env.tok)
    try:
        for cap in (exact - 1, 0):
            rc, got, text, toff, status = _device_run(ctx, lines, "NFKC", cap)
            assert rc == _lib.KGPU_ERR_CAPACITY and got == exact
            assert (text == 0x5A).all(), "a call that reports KGPU_ERR_CAPACITY wrote text"
        for cap in (exact, exact + 37):
            rc, got, text, toff, status = _device_run(ctx, lines, "NFKC", cap)
            assert rc == _lib.KGPU_OK and got == exact
            assert text[:exact].tobytes() == want_text.tobytes() and (text[exact:] == 0x5A).all()
            assert np.array_equal(toff, want_off) and np.array_equal(status, want_status)
        # the host forms: the exact size, and one more call with it succeeds (the binding's retry), or KgpuError for caller-owned arrays
        from kanpyo_amd.tokenizer import pack_sentences

        utf8, offs = pack_sentences(lines)
        assert env.tok.normalize_packed(utf8, offs)[0].tobytes() == want_text.tobytes()   # (first capacity 2 x the input: the retry runs)
        out = (np.full(exact - 1, 0x5A, dtype=np.uint8), np.zeros(5, dtype=np.uint64), np.zeros(4, dtype=np.uint8))
        with pytest.raises(_lib.KgpuError) as err:
            env.tok.normalize_packed(utf8, offs, out=out)
        assert err.value.code == _lib.KGPU_ERR_CAPACITY and (out[0] == 0x5A).all()
        got = C.c_uint64(0)
        assert _lib.lib().kgpu_normalize_batch(env.tok.handle, 2, utf8.ctypes.data, offs.ctypes.data, 4, out[0].ctypes.data, exact - 1, out[1].ctypes.data, out[2].ctypes.data,
                                               C.byref(got)) == _lib.KGPU_ERR_CAPACITY and got.value == exact
    finally:
        ctx.close()


# ---- 6. the device-resident chain --------------------------------------------------------------------------------------------------------------------------------


def test_device_chain_and_encode_tensor(env):
    import torch

    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    words = env.tok.words()
    vocab = words.vocabulary(["<unk>", "<s>"] + env.keys, unk_id=0, bos_id=1)
    host_norm = [N.host(s.encode(), "NFKC")[1] for s in SENTENCES]
    want_ids, want_off, want_status = vocab.encode_packed(*pack_sentences(host_norm))
    assert len(set(want_ids.tolist())) > 5 and (want_ids > 1).sum() > 50
    # by hand: normalize -> sync_normalize -> tokenize -> sync -> encode -> sync_lines, everything in device memory
    utf8, offs = pack_sentences(SENTENCES)
    n, total = len(SENTENCES), int(offs[-1])
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    cap = 11 * total
    d_norm = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_noff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_nst = torch.zeros(n, dtype=torch.uint8, device=dev)
    ctx = DeviceContext(env.tok)
    try:
        torch.cuda.synchronize(dev)
        ctx.normalize(d_utf8.data_ptr(), d_off.data_ptr(), n, d_norm.data_ptr(), cap, d_noff.data_ptr(), d_nst.data_ptr(), "NFKC")
        nbytes = ctx.sync_normalize()
        assert nbytes == sum(map(len, host_norm))
        tcap = nbytes + n + 64
        d_tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev)
        d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.tokenize(d_norm.data_ptr(), d_noff.data_ptr(), n, nbytes, d_tok.data_ptr(), tcap, d_toff.data_ptr(), d_st.data_ptr())
        n_tok = ctx.sync()
        d_ids = torch.empty(n_tok + n + 1, dtype=torch.int32, device=dev)
        d_ioff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        ctx.encode(vocab, d_norm.data_ptr(), d_noff.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_ids.data_ptr(), n_tok + n + 1, d_ioff.data_ptr())
        count = ctx.sync_lines()
        assert np.array_equal(d_ioff.cpu().numpy().view(np.uint64), want_off) and np.array_equal(d_ids[:count].cpu().numpy(), want_ids)
        assert np.array_equal(d_st.cpu().numpy(), want_status) and d_nst.cpu().numpy().tolist() == [4 if s.endswith("\u0301") else 0 for s in SENTENCES]
    finally:
        ctx.close()
    # Vocab.encode_tensor does the same by itself, from the keyword or from the Words handle's form
    merged = want_status.copy()
    merged[(merged == 0) & np.array([s.endswith("\u0301") for s in SENTENCES])] = 4
    nwords = env.tok.words(normalize="NFKC")
    nvocab = nwords.vocabulary(["<unk>", "<s>"] + env.keys, unk_id=0, bos_id=1)
    for v, kw in ((vocab, {"normalize": "NFKC"}), (nvocab, {})):
        ids, ioff, status = v.encode_tensor(SENTENCES, **kw)
        assert ids.is_cuda and np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(ioff.cpu().numpy().view(np.uint64), want_off)
        assert np.array_equal(status.cpu().numpy(), merged)
    ids, ioff, status = nvocab.encode_packed(utf8, offs)
    assert np.array_equal(ids, want_ids) and np.array_equal(ioff, want_off) and np.array_equal(status, merged)
    plain = vocab.encode_tensor(SENTENCES)[0].cpu().numpy()
    assert not np.array_equal(plain, want_ids)   # (without the form the half-width lines match no key)
    for h in (nvocab, nwords, vocab, words):
        h.close()


# ---- 7. a raw block, and the CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_raw_block(env):
    from kanpyo_amd.tokenizer import split_lines

    lines = mixed_lines(700, seed=7)
    block = b"".join(ln + [b"\n", "　\n".encode(), b" \t\r\n", "　　\n".encode()][i % 4] for i, ln in enumerate(lines)) + "ｶﾞ最後の行ＡＢＣ".encode()
    packed, offs = split_lines(block)
    raw, o = packed.tobytes(), offs.tolist()
    want_text, want_off, want_status = N.host_lines([raw[o[i] : o[i + 1]] for i in range(len(o) - 1)], "NFKC")
    text, toff, status = env.tok.normalize_text(block, "NFKC")
    assert len(status) == 701 and np.array_equal(toff, want_off) and np.array_equal(status, want_status) and text.tobytes() == want_text.tobytes()
    assert text.tobytes().endswith("ガ最後の行ABC".encode())
    text, toff, status = env.tok.normalize_text(b"", "NFC")
    assert len(text) == 0 and toff.tolist() == [0] and len(status) == 0


def test_cli(env, tmp_path):
    from kanpyo_amd.dictfile import DictFile, save_dict

    path = tmp_path / "t.dict"
    save_dict(DictFile(env.dict, env.known, env.unk), str(path))
    data = "ﾊﾝｶｸＡＢＣ㈱　\nテスト辞書\n\nｶﾞ東京１２３ \n".encode() * 40 + "形態素ﾊﾝｶｸ".encode()
    envv = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda argv, inp=data: subprocess.run([sys.executable, "-m", "kanpyo_amd"] + argv, input=inp, capture_output=True, env=envv, cwd=ROOT, timeout=600)   # noqa: E731
    outs = {}
    for split in ("host", "device"):
        r = run(["wakati", "-c", str(path), "--normalize", "nfkc", "--split", split, "--block-bytes", "500"])
        assert r.returncode == 0, r.stderr.decode()
        outs[split] = r.stdout
    assert outs["host"] == outs["device"] == "ハンカク ABC (株)\nテスト 辞書\n\nガ 東京 123\n".encode() * 40 + "形態素 ハンカク\n".encode()
    r = run(["wakati", "-c", str(path), "--split", "device"])
    assert r.returncode == 0 and r.stdout.startswith("\nテスト 辞書\n".encode())   # without it the half-width line has no words
    r = run(["wakati", "-c", str(path), "--normalize", "nfkc", "ﾊﾝｶｸＡＢＣ㈱"], b"")
    assert r.returncode == 0 and r.stdout == "ハンカク ABC (株)\n".encode()
    r = run(["tokenize", "-c", str(path), "--normalize", "nfkc", "ＡＢＣ"], b"")
    assert r.returncode == 0 and r.stdout.startswith("ABC\t名詞\nEOS".encode())
    # the normalize subcommand: the lines themselves; a status-4 line unchanged with a warning; an invalid line ends the run with 101
    long_line = ("a" + "\u0301" * 65).encode()
    for split in ("host", "device"):
        r = run(["normalize", "-c", str(path), "--split", split], "ﾊﾝｶｸ ＡＢＣ\n".encode() + long_line + b"\n\n" + "㈱\n".encode())
        assert r.returncode == 0 and r.stdout == "ハンカク ABC\n".encode() + long_line + "\n\n(株)\n".encode() and "line 2:" in r.stderr.decode(), split
        r = run(["normalize", "-c", str(path), "--split", split, "--form", "nfc"], "ＡＢＣe\u0301\n".encode() + b"\xff\n" + "never\n".encode())
        assert r.returncode == 101 and r.stdout == "ＡＢＣ\u00e9\n".encode() and "UTF-8" in r.stderr.decode(), split
    r = run(["graphviz", "-c", str(path), "--normalize", "nfkc", "ＡＢＣ"], b"")
    assert r.returncode == 0 and b"ABC" in r.stdout and "ＡＢＣ".encode() not in r.stdout


# ---- 8. the status of a call over normalised text ------------------------------------------------------------------------------------------------------------------
def test_status_merge(env):
    from kanpyo_amd.tokenizer import pack_sentences

    lines = ["ﾊﾝｶｸＡＢＣ".encode(), b"\xe3\x81", "テスト".encode(), ("a" + "\u0301" * 65).encode(), "ｶﾞ東京".encode(), b""]
    words = env.tok.words()
    utf8, offs = pack_sentences(lines)
    text, toff, status = words.render_packed(utf8, offs, normalize="NFKC")
    assert status.tolist() == [0, 1, 0, 4, 0, 0]
    pre = [N.host(ln, "NFKC")[1] for ln in lines]
    assert pre[1] == lines[1] and pre[3] == lines[3]
    ptext, ptoff, pstatus = words.render_packed(*pack_sentences(pre))
    assert pstatus.tolist() == [0, 1, 0, 0, 0, 0] and np.array_equal(toff, ptoff) and text.tobytes() == ptext.tobytes()
    raw, o = text.tobytes(), toff.tolist()
    assert raw[o[0] : o[1]] == "ハンカク ABC\n".encode() and raw[o[4] : o[5]] == "ガ 東京\n".encode()
    toks = env.tok.tokenize_batch(["ＡＢＣ東京"], normalize="NFKC")[0]
    assert [(t.surface, t.position) for t in toks[:2]] == [("ABC", 0), ("東京", 3)] and toks[-1].surface == "EOS" and len(toks) == 3   # positions in the normalised sentence
    lt, _, ls = env.tok.tokenize_lines_packed(utf8, offs, normalize="NFKC")
    assert ls.tolist() == [0, 1, 0, 4, 0, 0] and lt.tobytes().startswith("ハンカク\t名詞\nABC\t名詞\nEOS".encode())
    counts = env.tok.words(normalize="NFKC").counter()
    assert counts.add_packed(utf8, offs).tolist() == [0, 1, 0, 4, 0, 0] and dict(counts.most_common())["ハンカク".encode()] == 1
    info0 = env.tok.info()["device_bytes"]
    env.tok.normalize(["x"])
    assert env.tok.info()["device_bytes"] == info0   # the tables went up once, with the first call
    counts.close()
    words.close()
