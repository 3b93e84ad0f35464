"""Lines cut into sentences on the device (kgpu_sentence.hip: kgpu_split_sentences_device / kgpu_ctx_sync_sentences, kgpu_split_sentences_batch,
Vocab.encode_tensor(split_sentences=True), `--sentences`).  Expected values come from the host kgpu_split_sentences_host, which test_sentences_cpu.py
pins against a plain-Python restatement with a bracket stack.  Byte-exact, no tolerance: text, all S + 1 offsets, every record, both counts.

The kernel's tile is 4096 bytes (256 lanes x 16-byte units, four wavefronts of 1024 bytes); the carry kernels walk one tile per thread up to 1024
tiles (4 MiB of text) and two from there on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sentence_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

TILE, WAVE, UNIT = 4096, 1024, 16
CANARY = 0x5A5AC3C35A5AC3C3
# dense in every class: terminators, brackets of both kinds, Space of every width, text, '.', and truncated / stray lead and continuation bytes
ALPHABET = [c.encode() for c in R.DEFAULT_TERMINATORS + R.OPENERS + R.CLOSERS + " \t　   " + "あいう漢字abc.．"] + [b"\xe3", b"\x80", b"\xef\xbc", b"\xe2\x80", b"\xc2", b"\x82"]


@pytest.fixture(scope="module")
def synth_tok():
    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return sd, tok, known, unk


@pytest.fixture(scope="module")
def ctx(synth_tok):
    from kanpyo_amd.device import DeviceContext

    c = DeviceContext(synth_tok[1])
    yield c
    c.close()


def _host(lines, **kw):
    from kanpyo_amd import split_sentences_host

    return split_sentences_host(*R.pack(lines), **kw)


def _dev(ctx, lines, shift=0, cap=None, base=0, **kw):
    """The lines through the device split -> (fits, S, bytes, text, offsets, records).  The text sits `shift` bytes behind a 16-byte boundary and the
    offsets start at `base`; the bytes of d_out behind the sentences, the words behind d_out_offsets[cap] and the records behind d_sents[cap - 1] must
    come back untouched -- all of them when the capacity is too small."""
    import torch

    from kanpyo_amd import SENTENCE_DTYPE, _lib

    dev = torch.device("cuda", 0)
    utf8, offs = R.pack(lines)
    n, total = len(lines), int(utf8.size)
    d_in = torch.zeros(total + shift + 32, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 16 == 0
    if total:
        d_in[shift : shift + total] = torch.from_numpy(utf8).to(dev)
    d_off = torch.from_numpy((offs + np.uint64(base)).view(np.int64)).to(dev)
    if cap is None:
        cap = total + n + 1
    d_out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_ooff = torch.from_numpy(np.full(cap + 9, CANARY, dtype=np.uint64).view(np.int64)).to(dev)
    d_rec = torch.from_numpy(np.full(2 * cap + 16, CANARY, dtype=np.uint64).view(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    ctx.split_sentences(d_in.data_ptr() + shift - base, d_off.data_ptr(), n, total, d_out.data_ptr(), d_ooff.data_ptr(), d_rec.data_ptr(), cap,
                        _lib.sentence_opts(kw.get("terminators"), kw.get("brackets", True)))
    fits, S, nbytes = ctx.try_sync_sentences()
    out, ooff, rec = d_out.cpu().numpy(), d_ooff.cpu().numpy().view(np.uint64), d_rec.cpu().numpy().view(np.uint64)
    wrote_s, wrote_b = (S, nbytes) if fits else (0, 0)
    assert (out[wrote_b:] == 0xAB).all(), "a store behind the packed sentences"
    assert (ooff[(wrote_s + 1 if fits else 0):] == CANARY).all(), "a store behind d_out_offsets[S]"
    assert (rec[2 * wrote_s:] == CANARY).all(), "a store behind the records"
    return fits, S, nbytes, out[:wrote_b], ooff[: wrote_s + 1].copy(), rec[: 2 * wrote_s].copy().view(SENTENCE_DTYPE)


def _same_as_host(ctx, lines, shift=0, base=0, **kw):
    want_text, want_off, want_rec = _host(lines, **kw)
    fits, S, nbytes, text, off, rec = _dev(ctx, lines, shift, base=base, **kw)
    where = (len(lines), shift, kw)
    assert fits and S == len(want_rec) and nbytes == want_text.size, where
    assert np.array_equal(off, want_off), where
    assert np.array_equal(rec, want_rec), where
    assert np.array_equal(text, want_text), where
    return S


def _random_lines(rng, n_lines, max_parts):
    lines = []
    for _ in range(n_lines):
        k = int(rng.integers(0, max_parts + 1)) if rng.random() > 0.15 else 0
        lines.append(b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=k)))
    return lines


# ---- 1. the degenerate batches, the examples, the crafted cases of the fixture -----------------------------------------------------------------
def test_degenerate_and_crafted(ctx):
    fits, S, nbytes, text, off, rec = _dev(ctx, [])
    assert fits and S == 0 and nbytes == 0 and off.tolist() == [0]
    for lines in ([b""], [b"a"], [b"!"], [b" "], [b"\xe3"], [b"", b"", b""], [b"", b"a!b", b""]):
        _same_as_host(ctx, lines)
    g = load_golden("fixture_sentences.json")
    for c in g["cases"]:
        kw = {k: c[k] for k in ("terminators", "brackets") if k in c}
        lines = [bytes.fromhex(c["line_hex"]) if "line_hex" in c else c["line"].encode()]
        _same_as_host(ctx, lines, **kw)
        fits, S, _, text, off, rec = _dev(ctx, lines, **kw)
        pieces = [text.tobytes()[int(off[i]) : int(off[i + 1])] for i in range(S)]
        assert pieces == [bytes.fromhex(p) for p in c["pieces_hex"]] if "pieces_hex" in c else pieces == [p.encode() for p in c["pieces"]], c
    # all crafted lines as ONE batch, with the offsets starting somewhere else than 0
    lines = [bytes.fromhex(c["line_hex"]) if "line_hex" in c else c["line"].encode() for c in g["cases"] if "terminators" not in c and "brackets" not in c]
    _same_as_host(ctx, lines, base=1000)


# ---- 2. the text 0..15 bytes behind a 16-byte boundary --------------------------------------------------------------------------------------------
def test_every_alignment(ctx):
    rng = np.random.default_rng(3)
    lines = _random_lines(rng, 40, 60)
    for shift in range(16):
        _same_as_host(ctx, lines, shift)
        _same_as_host(ctx, lines[:3], shift, base=7)


# ---- 3. a line across one, two and three tile boundaries; brackets that match, and that do not, on either side of a boundary ---------------------
def test_lines_across_tiles(ctx):
    a = lambda k: b"a" * k   # noqa: E731
    inner = "中。また中！".encode()
    for crossings in (1, 2, 3):
        span = TILE * crossings
        # an opener in the first tile, its closer in the last: nothing inside is a boundary; behind the closer everything is
        _same_as_host(ctx, [b"x(" + a(TILE // 2) + inner + a(span - TILE // 2) + inner + b")y. z! w" + a(50) + "。終".encode()])
        # the opener never closes: every terminator of the line is a boundary
        _same_as_host(ctx, [b"x(" + a(TILE // 2) + inner + a(span) + inner + "。終".encode()])
        # a closer with nothing open, then a matched pair across the tiles
        _same_as_host(ctx, [b"x)" + inner + b"[" + a(span) + inner + b"]" + inner])
    for at in (TILE - 2, TILE - 1, TILE, TILE + 1):   # an unmatched opener / closer right at a tile boundary, terminators on both sides
        for br in (b"(", b")", "「".encode(), "」".encode()):
            _same_as_host(ctx, [a(at - 8) + "前。 ".encode()[: 8] + br + "後。次！".encode() + a(TILE) + b"?" + a(3)])
            _same_as_host(ctx, [b"(" + a(at - 9) + "前。 ".encode()[: 8] + br + "後。次！".encode() + a(TILE) + b")?" + a(3)])
    # nested and crossed kinds over three tiles, with a second line behind (its depth starts at 0 again)
    _same_as_host(ctx, ["「（".encode() + a(TILE) + "。」".encode() + a(TILE) + "！)".encode() + a(TILE) + "。終".encode(), "次（注。）。終".encode()])


# ---- 4. a terminator run, a three-byte terminator or bracket, inter-sentence Space at every offset across a unit, wavefront and tile boundary ------
def test_sweeps_across_unit_wave_and_tile(ctx):
    patterns = ["！？。次".encode(), "。次".encode(), "（。）。次".encode(), "。」次。".encode(), "。 　\t 次".encode(), "！　　　".encode(), "?!?! x".encode(),
                "「。".encode(), b"\xe3\x80\xe3\x80\x82\xe3" + "次".encode()]
    L = 2 * TILE   # every line is two tiles long, so line k starts at tile 2 k and its pattern sits at the same place in it
    for boundary in (4 * UNIT, WAVE, TILE):
        for pos in range(boundary - 16, boundary + 16):
            lines = [b"a" * pos + p + b"b" * (L - pos - len(p)) for p in patterns]
            assert all(len(x) == L for x in lines)
            _same_as_host(ctx, lines)
    # Space up to the line's end stays; the same Space in front of more text goes
    for pos in range(TILE - 16, TILE + 16):
        _same_as_host(ctx, [b"a" * pos + "。".encode() + "　".encode() * 9, b"a" * (TILE - 31) + "。".encode() + "　".encode() * 9 + b"z"])


# ---- 5. more line starts inside one tile than the tile has lanes; a tile without a line start; Space over whole tiles ----------------------------
def test_many_line_starts_and_none(ctx):
    for empties in (257, 300, 5000):
        _same_as_host(ctx, [b"a!b"] + [b""] * empties + ["次。終".encode()] + [b""] * 3)
    _same_as_host(ctx, [b""] * 1000)
    _same_as_host(ctx, [b"x", b"y"] * 700)                       # 1400 one-byte lines: 1400 starts in one tile
    _same_as_host(ctx, [b"a" * (5 * TILE + 77)])                  # tiles 1..4 have no line start and no event of any kind
    _same_as_host(ctx, [b"a." + b" " * (3 * TILE) + b"!" + b" " * (2 * TILE + 5) + b"z", b"q?" + b" " * (2 * TILE)])   # pending Space over whole tiles: dropped, then kept
    _same_as_host(ctx, [b"(" * (2 * TILE) + "。".encode() + b")" * TILE + "。次".encode() + b")" * (TILE + 3) + "。終".encode()])   # depths beyond a tile's bytes


# ---- 6. seeded random batches of some tens of kilobytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_batches(ctx, seed):
    rng = np.random.default_rng(seed)
    lines = _random_lines(rng, 300, 120) + [b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=6000))]
    assert 30_000 < sum(map(len, lines)) < 120_000
    _same_as_host(ctx, lines, shift=seed)
    _same_as_host(ctx, lines, brackets=False)
    _same_as_host(ctx, lines, terminators=".あ\U0001F600")


# ---- 7. one block just large enough for the carry kernels' second tile per thread: 1025 tiles, 4 MiB + 4 KiB -----------------------------------
def test_second_carry_round(ctx):
    rng = np.random.default_rng(11)
    piece = b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=20000))
    body = (piece * (1 + (1025 * TILE) // len(piece)))[: 1025 * TILE - 300]
    cut = len(body) // 3
    # one bracket pair around the first third, an opener that never closes in the second line, many lines in the third
    lines = ["（".encode() + body[:cut] + "）。終".encode(), "「".encode() + body[cut : 2 * cut]] + [body[k : k + 997] for k in range(2 * cut, len(body), 997)]
    total = sum(map(len, lines))
    assert 1024 * TILE < total <= 1025 * TILE
    _same_as_host(ctx, lines, shift=9)


# ---- 8. a capacity one too small ----------------------------------------------------------------------------------------------------------------------
def test_capacity_one_too_small(ctx):
    rng = np.random.default_rng(5)
    lines = _random_lines(rng, 120, 80)
    want = len(_host(lines)[2])
    fits, S, _, text, off, rec = _dev(ctx, lines, cap=want - 1)   # (_dev checks that nothing at all was stored)
    assert not fits and S == want
    fits, S, _, *_ = _dev(ctx, lines, cap=want)
    assert fits and S == want
    fits, S, *_ = _dev(ctx, [b""], cap=0)
    assert not fits and S == 1


# ---- 9. the host-memory call, across chunk boundaries ---------------------------------------------------------------------------------------------------
def test_batch_across_chunks(synth_tok, monkeypatch):
    tok = synth_tok[1]
    rng = np.random.default_rng(8)
    lines = _random_lines(rng, 200, 60)
    want = _host(lines)
    for hook in ({}, {"KGPU_HOST_CHUNK_BYTES": "700"}, {"KGPU_HOST_CHUNK_SENTS": "7"}):
        for k, v in hook.items():
            monkeypatch.setenv(k, v)
        got = tok.split_sentences_packed(*R.pack(lines))
        for k in hook:
            monkeypatch.delenv(k)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), hook
    assert tok.split_sentences(["彼は「行く。」と言った。次の文！？ 最後", "", b"a!b"]) == [["彼は「行く。」と言った。", "次の文！？", "最後"], [""], [b"a!", b"b"]]
    assert tok.split_sentences(["a.b。c"], terminators=".") == [["a.", "b。c"]]
    assert tok.split_sentences(["（a。b）c"], brackets=False) == [["（a。", "b）c"]]


# ---- 10. encode_tensor over documents equals encode_tensor over the host function's sentences -------------------------------------------------------------
def test_encode_tensor_split_sentences(synth_tok):
    from kanpyo_amd import split_sentences_host, synth
    from kanpyo_amd.tokenizer import normalize_host

    sd, tok, *_ = synth_tok
    sents = synth.make_corpus(sd, 120, 4, "cfg2")
    toks, toff, _ = tok.tokenize_packed(*R.pack([s.encode() for s in sents]))
    raw = "".join(sents).encode()
    vocab = [b"<unk>", b"<s>", b"</s>"] + sorted({s.encode()[int(t["position"]) : int(t["position"]) + int(t["byte_len"])] for i, s in enumerate(sents)
                                                 for t in toks[int(toff[i]) : int(toff[i + 1])] if int(t["byte_len"])})[:400]
    del raw
    v = tok.words().vocabulary(vocab, 0, 1, 2)
    marks = ["。", "！？", "！", "｡ ", "。　", "?"]
    docs = ["".join(s + marks[(i + j) % len(marks)] for j, s in enumerate(sents[i : i + 7])) for i in range(0, len(sents), 7)] + ["", "（" + sents[0] + "。" + sents[1] + "）" + sents[2]]
    for form in (None, "NFKC"):
        lines = [normalize_host(d, form) if form else d.encode() for d in docs]
        text, off, rec = split_sentences_host(*R.pack(lines))
        pieces = [text.tobytes()[int(off[k]) : int(off[k + 1])] for k in range(len(rec))]
        ids, ioff, st, sent = v.encode_tensor(docs, normalize=form, split_sentences=True)
        wids, woff, wst = v.encode_tensor(pieces)
        assert ids.cpu().tolist() == wids.cpu().tolist() and ioff.cpu().tolist() == woff.cpu().tolist() and st.cpu().tolist() == wst.cpu().tolist(), form
        assert sent.cpu().numpy().tolist() == [[int(r["line"]), int(r["byte_start"]), int(r["char_start"])] for r in rec], form
        pids, plen, pst, psent = v.encode_tensor(docs, width=12, pad_id=-1, normalize=form, split_sentences=True)
        wpids, wplen, _ = v.encode_tensor(pieces, width=12, pad_id=-1)
        assert pids.cpu().tolist() == wpids.cpu().tolist() and plen.cpu().tolist() == wplen.cpu().tolist() and psent.cpu().tolist() == sent.cpu().tolist(), form
    with pytest.raises(ValueError):
        v.encode_tensor(docs, split_sentences=True, return_spans=True)


# ---- 11. `wakati --sentences` equals `wakati` fed the host function's sentences ------------------------------------------------------------------------------
def test_cli_wakati_sentences(synth_tok, tmp_path):
    from kanpyo_amd import split_sentences_host, synth
    from kanpyo_amd.dictfile import DictFile, save_dict

    sd, _, known, unk = synth_tok
    path = tmp_path / "t.dict"
    save_dict(DictFile(sd.dict, known, unk), str(path))
    sents = synth.make_corpus(sd, 40, 9, "cfg2")
    docs = ["".join(s + "。" for s in sents[i : i + 5]) for i in range(0, 40, 5)] + ["「" + sents[0] + "！" + sents[1] + "」" + sents[2] + "？ " + sents[3]]
    data = "".join(d + "\n" for d in docs).encode()
    text, off, rec = split_sentences_host(*R.pack([d.encode() for d in docs]))
    fed = b"".join(text.tobytes()[int(off[k]) : int(off[k + 1])] + b"\n" for k in range(len(rec)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "wakati", "-c", str(path)]
    a = subprocess.run(cmd + ["--sentences"], input=data, capture_output=True, env=env, cwd=ROOT, timeout=600)
    b = subprocess.run(cmd, input=fed, capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr.decode(), b.stderr.decode())
    assert a.stdout == b.stdout and a.stdout.count(b"\n") == len(rec) > len(docs)
