"""read_line + trim_end on the device (kgpu_split.hip: kgpu_split_lines_device / kgpu_ctx_sync_split) and the raw-block entry point on top of
it (kgpu_tokenize_text_lines, Tokenizer.tokenize_text_lines, `--split device`).  Expected values come from the host kgpu_split_lines (pinned on the
CPU by test_lines_cpu.py) and, for the small cases, from a restatement of read_line + str::trim_end written here.  Byte-exact, no tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, fixture_dict_parts, load_golden

pytestmark = pytest.mark.gpu

# char::is_whitespace: the Unicode White_Space property, 25 code points
WHITE_SPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(map(chr, range(0x2000, 0x200B))) + "\u2028\u2029\u202f\u205f\u3000"
assert len(WHITE_SPACE) == 25
# the whitespace-heavy alphabet: every White_Space code point, look-alikes that are not space, truncated / stray lead and continuation bytes
ALPHABET = [c.encode() for c in WHITE_SPACE + "\x1c\x1d\x1e\x1fa\u3042\u6f22\u200b"] + [b"\xff", b"\xe3", b"\x80", b"\xc2", b"\xe2\x80", b"\r\n"]
CANARY = 0x5A5AC3C35A5AC3C3
MIB = 1 << 20


def _ref_split(b: bytes):
    """read_line (up to and including '\\n'; the last line may lack it) + trim_end; invalid bytes are never White_Space."""
    if not b:
        return []
    parts = b.split(b"\n")
    if b.endswith(b"\n"):
        parts.pop()
    return [p.decode("utf-8", "surrogateescape").rstrip(WHITE_SPACE).encode("utf-8", "surrogateescape") for p in parts]


def _pack(lines):
    return b"".join(lines), np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)


def _host(block):
    from kanpyo_amd.tokenizer import split_lines

    text, offs = split_lines(block)
    return text, offs


@pytest.fixture(scope="module")
def synth_full():
    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return sd, tok, known, unk


@pytest.fixture(scope="module")
def ctx(synth_full):
    from kanpyo_amd.device import DeviceContext

    c = DeviceContext(synth_full[1])
    yield c
    c.close()


def _dev_split(ctx, block, shift=0, cap=None):
    """The block through the device split -> (packed uint8 array, offsets uint64 array).  The input sits `shift` bytes behind a 16-byte boundary;
    the bytes of d_out behind the packed lines and the words behind d_offsets[cap] must come back untouched."""
    import torch

    dev = torch.device("cuda", 0)
    src = np.frombuffer(bytes(block), dtype=np.uint8) if not isinstance(block, np.ndarray) else block
    n = int(src.size)
    d_in = torch.zeros(n + shift + 16, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 16 == 0
    if n:
        d_in[shift : shift + n] = torch.from_numpy(src.copy()).to(dev)
    d_out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
    if cap is None:
        cap = int(np.count_nonzero(src == 10)) + 2
    d_off = torch.from_numpy(np.full(cap + 8, CANARY, dtype=np.uint64).view(np.int64)).to(dev)
    ctx.split_lines(d_in.data_ptr() + shift, n, d_out.data_ptr(), d_off.data_ptr(), cap)
    n_lines, n_bytes = ctx.sync_split()
    out = d_out.cpu().numpy()
    off = d_off.cpu().numpy().view(np.uint64)
    assert (out[n_bytes:] == 0xAB).all(), "a store behind the packed lines"
    assert (off[cap:] == CANARY).all(), "a store behind d_offsets[capacity]"
    return out[:n_bytes], off[: n_lines + 1].copy()


def _same_as_host(ctx, block, shift=0):
    want, want_off = _host(block)
    got, got_off = _dev_split(ctx, block, shift)
    assert np.array_equal(got_off, want_off)
    assert np.array_equal(got, want)


def _lines(ctx, b: bytes, shift=0):
    text, offs = _dev_split(ctx, b, shift)
    t = text.tobytes()
    return [t[int(offs[i]) : int(offs[i + 1])] for i in range(len(offs) - 1)]


# ---- 1. the case table of the host splitter ---------------------------------------------------------------------------------------------
def test_case_table(ctx):
    s = lambda b: _lines(ctx, b)   # noqa: E731
    assert s(b"") == []
    assert s(b"\n") == [b""]
    assert s(b"a") == [b"a"] and s(b"a\n") == [b"a"] and s(b"a\n\n") == [b"a", b""]
    assert s("すもも\r\nもも \u3000\n  \t\nlast".encode()) == ["すもも".encode(), "もも".encode(), b"", b"last"]
    for ws in WHITE_SPACE.replace("\n", ""):
        assert s(("x" + ws + ws + "\n").encode()) == [b"x"], hex(ord(ws))
        assert s((ws + "x").encode()) == [(ws + "x").encode()], hex(ord(ws))          # leading space is kept
    for keep in "\x1c\x1d\x1e\x1f\u200b\ufeff\x00":
        assert s(("x" + keep).encode()) == [("x" + keep).encode()], hex(ord(keep))
    # invalid bytes before and inside trailing space: only complete encodings go
    assert s(b"x\xff \xe3\x80\x80") == [b"x\xff"]
    assert s(b"x\xe3\x80") == [b"x\xe3\x80"]            # a truncated U+3000 stays
    assert s(b"x\xe3\xe3\x80\x80") == [b"x\xe3"]
    assert s(b"x\xc2 \xc2\x85") == [b"x\xc2"]
    assert s(b"\x80\x20") == [b"\x80"]
    assert s(b"x\r\n") == [b"x"] and s(b"\r\n\r\n") == [b"", b""]


# ---- 2. every small length, the degenerate blocks ---------------------------------------------------------------------------------------
def test_every_length_to_64_and_degenerate_blocks(ctx):
    rng = np.random.default_rng(17)
    stream = b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=200))
    for n in range(0, 65):
        for shift in (0, 5):
            b = stream[:n]
            want = _ref_split(b)
            assert _lines(ctx, b, shift) == want, (n, shift, b)
            text, offs = _dev_split(ctx, b, shift)
            assert offs[0] == 0 and len(offs) == len(want) + 1
    text, offs = _dev_split(ctx, b"")
    assert text.size == 0 and offs.tolist() == [0]
    assert _lines(ctx, "改行のないブロック \u3000".encode()) == ["改行のないブロック".encode()]
    for n in (1, 63, 64, 65, 4096, 4097, 16384, 16385, 40000):
        text, offs = _dev_split(ctx, b"\n" * n)
        assert text.size == 0 and len(offs) == n + 1 and not offs.any()
    assert _lines(ctx, b"ab\ncd\n") == [b"ab", b"cd"] and _lines(ctx, b"ab\ncd") == [b"ab", b"cd"] and _lines(ctx, b"ab\ncd \n ") == [b"ab", b"cd", b""]


# ---- 3. random blocks, tile edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_blocks_of_a_mebibyte(ctx, seed):
    rng = np.random.default_rng(seed)
    block = b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=MIB // 2 + 30000))   # ~1 MiB: the entries average ~2 bytes
    assert MIB * 0.9 < len(block) < MIB * 1.6
    _same_as_host(ctx, block, shift=seed % 3 * 7)
    if seed == 1:   # ... and the restatement itself on a prefix
        assert _lines(ctx, block[:50000]) == _ref_split(block[:50000])


def test_every_encoding_byte_meets_a_tile_edge(ctx):
    tile = 4096   # kgpu_split.hip: TILE, a multiple of 16
    line = ("x" + "\u3000" * 3 + "\n").encode()   # 11 bytes
    for pad in range(48):
        block = b"a" * pad + line * (3 * tile // len(line) + 8)
        assert len(block) >= 3 * tile
        _same_as_host(ctx, block)


# ---- 4. carries across many tiles ---------------------------------------------------------------------------------------------------------
def test_long_carries(ctx):
    ideo = "\u3000".encode()
    _same_as_host(ctx, "行".encode() + ideo * (MIB // 3) + b"\nnext \n")
    got, off = _dev_split(ctx, "行".encode() + ideo * (MIB // 3) + b"\n")
    assert got.tobytes() == "行".encode() and off.tolist() == [0, 3]
    got, off = _dev_split(ctx, b" " * MIB)   # one line, nothing kept
    assert got.size == 0 and off.tolist() == [0, 0]
    _same_as_host(ctx, b" " * MIB + b"x")      # ... and all of it kept: leading space
    _same_as_host(ctx, b"a" * MIB + b"\n" + b"bc \ndef\n\n" * 100)
    _same_as_host(ctx, b"a" * MIB + ideo * 5000 + b"\n" + b"bc \ndef\n\n" * 100, shift=9)


def test_carries_across_the_carry_kernels_rounds(ctx):
    """The carry kernel takes the tiles in rounds of thousands (kgpu_split.hip): runs of spaces and lines that span several rounds (40 MiB = 10240 tiles, 8192 to a round)."""
    big = 40 * MIB
    got, off = _dev_split(ctx, b"y" + b" " * big + b"\nz \n")
    assert got.tobytes() == b"yz" and off.tolist() == [0, 1, 2]
    got, off = _dev_split(ctx, b"\n" + b" " * big + b"x" + b" " * MIB, shift=3)   # kept: the spaces lead the line
    assert off.tolist() == [0, 0, big + 1] and got.size == big + 1 and got[-1] == ord("x") and (got[:-1] == 32).all()
    _same_as_host(ctx, b"a" * big + "\u3000".encode() * MIB + b"\nshort\t\n\n")


# ---- 5. one large block -------------------------------------------------------------------------------------------------------------------
def test_large_block_64_mib(ctx, synth_full):
    from kanpyo_amd import synth

    sd = synth_full[0]
    sents = synth.make_corpus(sd, 64 * MIB // 112 + 20000, 21, "cfg2")
    tails = ["\n", "\r\n", "\u3000\n"]
    block = "".join(s + tails[i % 3] for i, s in enumerate(sents)).encode()
    assert len(block) >= 64 * MIB
    block = np.frombuffer(block, dtype=np.uint8)[: 64 * MIB]
    _same_as_host(ctx, block)


# ---- 6. protocol --------------------------------------------------------------------------------------------------------------------------
def test_capacity_overlap_and_size_checks(ctx, synth_full):
    import torch

    from kanpyo_amd import _lib

    dev = torch.device("cuda", 0)
    block = "one \ntwo\n\nfour\u3000\nlast".encode()
    src = np.frombuffer(block, dtype=np.uint8)
    want, want_off = _host(block)
    assert len(want_off) == 6
    d_in = torch.from_numpy(src.copy()).to(dev)
    d_out = torch.full((src.size + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(np.full(16, CANARY, dtype=np.uint64).view(np.int64)).to(dev)
    # one entry short: the count is reported, nothing behind the capacity or behind d_out[len] is touched
    ctx.split_lines(d_in.data_ptr(), src.size, d_out.data_ptr(), d_off.data_ptr(), 5)
    L = _lib.lib()
    n, b = C.c_uint64(0), C.c_uint64(0)
    assert L.kgpu_ctx_sync_split(ctx._h, C.byref(n), C.byref(b)) == _lib.KGPU_ERR_CAPACITY and n.value == 5
    assert (d_off.cpu().numpy().view(np.uint64)[5:] == CANARY).all() and (d_out.cpu().numpy()[src.size :] == 0xAB).all()
    # exactly enough
    ctx.split_lines(d_in.data_ptr(), src.size, d_out.data_ptr(), d_off.data_ptr(), 6)
    assert ctx.sync_split() == (5, len(want))
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64)[:6], want_off) and (d_off.cpu().numpy().view(np.uint64)[6:] == CANARY).all()
    assert d_out.cpu().numpy()[: len(want)].tobytes() == want.tobytes() and (d_out.cpu().numpy()[len(want) :] == 0xAB).all()
    # nothing pending: zeros
    assert ctx.sync_split() == (0, 0)
    # overlap of d_in and d_out, whole or by one byte at either end
    for d_o in (d_in.data_ptr(), d_in.data_ptr() + src.size - 1, d_in.data_ptr() - src.size + 1):
        with pytest.raises(_lib.KgpuError) as e:
            ctx.split_lines(d_in.data_ptr(), src.size, d_o, d_off.data_ptr(), 6)
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "overlap" in str(e.value)
    # 4 GiB and more: an argument check, nothing is allocated or launched
    for size in (1 << 32, (1 << 32) + 5, 1 << 40):
        with pytest.raises(_lib.KgpuError) as e:
            ctx.split_lines(d_in.data_ptr(), size, d_out.data_ptr(), d_off.data_ptr(), 6)
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    assert ctx.sync_split() == (0, 0)
    # null pointers
    with pytest.raises(_lib.KgpuError) as e:
        ctx.split_lines(0, 4, d_out.data_ptr(), d_off.data_ptr(), 6)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    with pytest.raises(_lib.KgpuError) as e:
        ctx.split_lines(d_in.data_ptr(), 4, d_out.data_ptr(), 0, 6)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    # capacity 0 with no table at all: the count still comes back
    ctx.split_lines(d_in.data_ptr(), src.size, d_out.data_ptr(), 0, 0)
    assert L.kgpu_ctx_sync_split(ctx._h, C.byref(n), C.byref(b)) == _lib.KGPU_ERR_CAPACITY and n.value == 5


def test_two_splits_back_to_back(ctx):
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    blocks = [b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=k)) for k in (60000, 9000)]
    bufs = []
    for blk in blocks:   # the second is enqueued while the first is pending: the context syncs the first before it reuses its control words
        src = np.frombuffer(blk, dtype=np.uint8)
        d_in = torch.from_numpy(src.copy()).to(dev)
        d_out = torch.full((src.size,), 0xAB, dtype=torch.uint8, device=dev)
        cap = blk.count(b"\n") + 2
        d_off = torch.zeros(cap, dtype=torch.int64, device=dev)
        ctx.split_lines(d_in.data_ptr(), src.size, d_out.data_ptr(), d_off.data_ptr(), cap)
        bufs.append((d_in, d_out, d_off))
    n_lines, n_bytes = ctx.sync_split()
    torch.cuda.synchronize()
    for k, blk in enumerate(blocks):
        want, want_off = _host(blk)
        _, d_out, d_off = bufs[k]
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64)[: len(want_off)], want_off)
        assert np.array_equal(d_out.cpu().numpy()[: len(want)], want)
        if k == 1:
            assert (n_lines, n_bytes) == (len(want_off) - 1, len(want))


def test_split_feeds_tokenize_device_without_leaving_hbm(ctx, synth_full):
    import torch

    from kanpyo_amd import synth
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    sd, tok, _, _ = synth_full
    sents = synth.make_corpus(sd, 3000, 31, "cfg2") + synth.make_corpus(sd, 40, 32, "cfg3")
    tails = ["\n", " \r\n", "\u3000 \n", "\t\n"]
    block = "".join(s + tails[i % 4] for i, s in enumerate(sents)).encode()
    utf8, offs = _host(block)
    want_tok, want_toff, want_st = tok.tokenize_packed(utf8, offs)
    dev = torch.device("cuda", 0)
    src = np.frombuffer(block, dtype=np.uint8)
    d_in = torch.from_numpy(src.copy()).to(dev)
    d_text = torch.empty(src.size, dtype=torch.uint8, device=dev)
    cap_off = block.count(b"\n") + 2
    d_off = torch.empty(cap_off, dtype=torch.int64, device=dev)
    ctx.split_lines(d_in.data_ptr(), src.size, d_text.data_ptr(), d_off.data_ptr(), cap_off)
    n, total = ctx.sync_split()
    assert (n, total) == (len(offs) - 1, len(utf8))
    cap = total + n + 1
    d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.tokenize(d_text.data_ptr(), d_off.data_ptr(), n, total, d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
    got = ctx.sync()
    assert got == len(want_tok)
    assert np.array_equal(d_toff.cpu().numpy().view(np.uint64), want_toff)
    assert np.array_equal(d_st.cpu().numpy(), want_st)
    assert np.array_equal(d_tok[:got].cpu().numpy().view(TOKEN_DTYPE).reshape(-1), want_tok)


# ---- 7. the raw-block entry point ---------------------------------------------------------------------------------------------------------
def _text_matches(tok, block):
    want = tok.tokenize_lines_packed(*_host(block))
    got = tok.tokenize_text_lines(block)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])
    assert got[0].tobytes() == want[0].tobytes()
    return want


def test_text_lines_on_the_fixture_dictionary():
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = fixture_dict_parts()
    tok = Tokenizer(Dict.from_parts(**p))
    tok.set_features(MorphFeatureTable.from_features([["名詞", f"k{i}", "*"] for i in range(1, len(p["morphs"]) + 1)]),
                     MorphFeatureTable.from_features([["未知語", f"u{i}"] for i in range(1, len(p["unk_morphs"]) + 1)]))
    inputs = [c["input"] for c in load_golden("fixture_tokens.json")["cases"]]
    ws = WHITE_SPACE.replace("\n", "")
    block = "".join(s + ws[i % len(ws)] * (i % 3) + "\n" for i, s in enumerate(inputs)).encode()
    want = _text_matches(tok, block)
    assert want[0].size and not want[2].any()
    _text_matches(tok, block[:-1])   # no final newline
    _text_matches(tok, b"")
    _text_matches(tok, b"\n")
    _text_matches(tok, b" \n\xff\n")


def test_text_lines_on_the_synthetic_dictionary(synth_full, monkeypatch):
    from kanpyo_amd import synth

    sd, tok, _, _ = synth_full
    sents = synth.make_corpus(sd, 21000, 41, "cfg2") + synth.make_corpus(sd, 21000, 42, "cfg3")
    rng = np.random.default_rng(43)
    order = rng.permutation(len(sents))
    ws = WHITE_SPACE.replace("\n", "")
    parts = []
    for k, i in enumerate(order):
        tail = "".join(ws[j] for j in rng.integers(0, len(ws), size=int(rng.integers(0, 4))))
        parts.append((sents[i] + tail + "\n").encode())
        if k % 5000 == 17:
            parts.append(b"\n")                               # an empty line
        if k == len(order) // 2:
            parts.append(b"\xe3\x81\xff\xfe \n")              # a line that is not UTF-8
        if k == len(order) // 3:
            parts.append(("長い行" * 11200).encode()[:99999] + "\u3000\n".encode())   # one line of ~100 000 bytes
    block = b"".join(parts)
    want = _text_matches(tok, block)
    assert len(want[1]) - 1 > 42000 and (want[2] == 1).sum() >= 1
    bad = int(np.flatnonzero(want[2] == 1)[0])
    assert want[1][bad] == want[1][bad + 1]                    # it renders to nothing, on its own line index
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "700")          # many more chunks than contexts
    _text_matches(tok, block[: 2 * MIB])


def test_text_lines_capacity_protocol(synth_full):
    from kanpyo_amd import _lib

    sd, tok, _, _ = synth_full
    # the wrapper's first offsets table is too small for a block of very short lines: it retries with the count the device found
    block = ("あ\n" * 6000).encode()
    want = _text_matches(tok, block)
    assert len(want[1]) == 6001
    # the C call: either buffer one short -> KGPU_ERR_CAPACITY with both exact sizes; exact -> KGPU_OK
    L = _lib.lib()
    block = "すもももももももものうち \nテスト\u3000\n\n最後".encode()
    text, toff, st = tok.tokenize_lines_packed(*_host(block))
    src = np.frombuffer(block, dtype=np.uint8)
    n_l, n_b = len(toff) - 1, len(text)
    for tcap, ocap in ((n_b - 1, n_l + 1), (n_b, n_l), (0, 0)):
        out = np.full(n_b + 8, 0xAB, dtype=np.uint8)
        offs = np.full(n_l + 4, CANARY, dtype=np.uint64)
        status = np.full(n_l + 4, 0xCD, dtype=np.uint8)
        n, b = C.c_uint64(0), C.c_uint64(0)
        rc = L.kgpu_tokenize_text_lines(tok.handle, src.ctypes.data, src.size, out.ctypes.data, tcap, offs.ctypes.data, ocap, status.ctypes.data, C.byref(n), C.byref(b))
        assert rc == _lib.KGPU_ERR_CAPACITY and (n.value, b.value) == (n_l, n_b), (tcap, ocap)
        assert (out[tcap:] == 0xAB).all() and (offs[ocap:] == CANARY).all() and (status[max(ocap - 1, 0) :] == 0xCD).all()
    out = np.full(n_b + 8, 0xAB, dtype=np.uint8)
    offs = np.full(n_l + 4, CANARY, dtype=np.uint64)
    status = np.full(n_l + 4, 0xCD, dtype=np.uint8)
    n, b = C.c_uint64(0), C.c_uint64(0)
    rc = L.kgpu_tokenize_text_lines(tok.handle, src.ctypes.data, src.size, out.ctypes.data, n_b, offs.ctypes.data, n_l + 1, status.ctypes.data, C.byref(n), C.byref(b))
    assert rc == _lib.KGPU_OK and (n.value, b.value) == (n_l, n_b)
    assert out[:n_b].tobytes() == text.tobytes() and (out[n_b:] == 0xAB).all()
    assert np.array_equal(offs[: n_l + 1], toff) and (offs[n_l + 1 :] == CANARY).all()
    assert np.array_equal(status[:n_l], st) and (status[n_l:] == 0xCD).all()
    # a handle without feature tables
    from kanpyo_amd import Tokenizer

    with pytest.raises(_lib.KgpuError) as e:
        Tokenizer(sd.dict).tokenize_text_lines(b"a\n")
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "kgpu_dict_set_features" in str(e.value)


# ---- 8. the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_split_device_writes_what_the_default_writes(synth_full, tmp_path):
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile, save_dict

    sd, tok, known, unk = synth_full
    path = tmp_path / "t.dict"
    save_dict(DictFile(sd.dict, known, unk), str(path))
    sents = synth.make_corpus(sd, 3000, 11, "cfg2")
    raw = [s + ["\r\n", "\u3000\n", " \t\n", "\n"][i % 4] for i, s in enumerate(sents)]
    raw.insert(5, "\n")
    data = "".join(raw).encode() + "最後の行".encode()
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path), "--block-bytes", "20000"]

    def run(split, stdin):
        return subprocess.run(cmd + (["--split", split] if split else []), input=stdin, capture_output=True, env=env, cwd=ROOT, timeout=600)

    base, host, dev = run(None, data), run("host", data), run("device", data)
    assert base.returncode == 0 and host.returncode == 0, base.stderr.decode() + host.stderr.decode()
    assert dev.returncode == 0, dev.stderr.decode()
    assert base.stdout.count(b"EOS\t\n") == len(raw) + 1
    assert host.stdout == base.stdout
    assert dev.stdout == base.stdout
    # an invalid line in the middle: the lines before it, then a panic's exit status -- on both
    cut = data.index(b"\n", len(data) // 2) + 1
    bad = data[:cut] + b"\xff\xfe\n" + data[cut:]
    host, dev = run("host", bad), run("device", bad)
    assert host.returncode == 101 and dev.returncode == 101
    assert 0 < len(host.stdout) < len(base.stdout) and base.stdout.startswith(host.stdout)
    assert dev.stdout == host.stdout
