"""The source alignment on the device (include/kanpyo_gpu.h, "source alignment"; kgpu_normalize.hip's ALIGN instantiations, kgpu_align.hip): the aligned
normalise calls, kgpu_source_spans_device / _batch, Tokenizer.tokenize_aligned and the CLI's `align`.  The expected value is always the host twin
(kgpu_normalize_host_aligned, kgpu_source_spans_host: pinned against unicodedata and the header's rules in tests/test_align_cpu.py) -- never the device's
own output.  No tolerance: bytes, offsets, status bytes, edit records and spans are compared exactly.

The write pass carries three more running sums from lane to lane and from 1024-byte pass to pass (edits, output and source code points): the position
test puts an edit across every 16-byte unit boundary and every pass boundary, and the 8 KiB all-half-width line has thousands of edits over many passes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import normalize_ref as N
from conftest import ROOT, load_golden
from kanpyo_amd import _lib
from normalize_cases import DAKUTEN, KA, SENTENCES, env, mixed_lines  # noqa: F401  (env: the fixture)

pytestmark = pytest.mark.gpu


def check_batch(tok, lines, form):
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(lines)
    text, toff, status, edits, eoff = tok.normalize_packed_aligned(utf8, offs, form)
    want_text, want_off, want_status, want_edits, want_eoff = A.host_lines_aligned(lines, form)
    assert np.array_equal(toff, want_off) and np.array_equal(status, want_status) and np.array_equal(eoff, want_eoff), form
    assert text.tobytes() == want_text.tobytes(), form
    assert edits.dtype == A.EDIT_DTYPE and edits.tobytes() == want_edits.tobytes(), form
    plain = tok.normalize_packed(utf8, offs, form)   # the unaligned twin: the same text
    assert plain[0].tobytes() == want_text.tobytes() and np.array_equal(plain[1], want_off) and np.array_equal(plain[2], want_status)
    return text, toff, status, edits, eoff


# ---- 1. the fixtures ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["NFC", "NFKC"])
def test_fixture_parity(env, form):
    _, cases = N.fixture_cases()
    g = load_golden("fixture_align.json")
    mine = [c for c in g["cases"] if c["form"] == form]
    lines = [raw for _, raw, _ in cases] + [bytes.fromhex(c["input"]) for c in mine]
    text, toff, status, edits, eoff = check_batch(env.tok, lines, form)
    assert 1 in status and 4 in status and 0 in status
    e = eoff.tolist()
    for i, st in enumerate(status.tolist()):
        if st:
            assert e[i] == e[i + 1]   # a line that is copied unchanged has no edits
    for k, c in enumerate(mine):
        i = len(cases) + k
        assert [list(t) for t in A.edit_tuples(edits[e[i] : e[i + 1]])] == c["edits"], c["name"]


# ---- 2. an edit across every unit and pass boundary ----------------------------------------------------------------------------------------------------
def test_positions(env):
    pads = list(range(0, 71)) + list(range(1000, 1041))
    lines = []
    for seg in ((KA + DAKUTEN).encode(), "e\u0301".encode(), (KA + DAKUTEN + "Ａ").encode()):
        lines += [b"p" * pad + seg for pad in pads] + [b"p" * pad + seg + b"q" for pad in pads]
    lines += [b"x" * 1023 + (KA + DAKUTEN).encode(), b"x" * 1024 + (KA + DAKUTEN).encode()]
    for form in ("NFC", "NFKC"):
        text, toff, status, edits, eoff = check_batch(env.tok, lines, form)
        assert not status.any()
    counts = np.diff(eoff.astype(np.int64))
    assert counts[: 4 * len(pads)].tolist() == [1] * (4 * len(pads)) and counts[4 * len(pads) : 6 * len(pads)].tolist() == [2] * (2 * len(pads)) and counts[-2:].tolist() == [1, 1]
    assert A.edit_tuples(edits[-1:]) == [(1024, 1024, 1024, 1024, 3, 6, 1, 2)]
    # behind an edit in an earlier pass: the carried bases
    lines = [("ｶﾞ" * 200 + "p" * pad + "ﾊﾟＡ").encode() for pad in range(0, 40)]
    text, toff, status, edits, eoff = check_batch(env.tok, lines, "NFKC")
    assert np.diff(eoff.astype(np.int64)).tolist() == [202] * 40


# ---- 3. batch shapes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 8200])
def test_batch_shapes(env, n):
    lines = mixed_lines(n, seed=300 + n, max_bytes=200 if n <= 4097 else 40)   # (8200: more lines than the launch has workgroups)
    if n >= 63:
        lines[n // 2] = ("ﾊﾝｶｸｶﾀｶﾅﾃﾞｽ" * 300).encode()[:8192 // 3 * 3]   # one 8 KiB line that is all half-width kana: thousands of edits, many passes
        lines[7] = b""
        lines[9] = b"\xffbad"
        lines[11] = ("a" + "\u0301" * 65).encode()
    text, toff, status, edits, eoff = check_batch(env.tok, lines, "NFKC")
    assert len(toff) == n + 1 and len(status) == n and len(eoff) == n + 1
    if n >= 63:
        e = eoff.tolist()
        assert status[9] == 1 and status[11] == 4 and e[9] == e[10] and e[11] == e[12] and e[7] == e[8] and e[n // 2 + 1] - e[n // 2] > 2400
        check_batch(env.tok, lines, "NFC")


# ---- 4. capacity on the device form ---------------------------------------------------------------------------------------------------------------------
def _device_run(ctx, lines, form, capacity, edit_capacity):
    """kgpu_normalize_device_aligned over torch tensors -> (rc, bytes, edits, text buffer, edit buffer as bytes -- 64 / 48 canary bytes behind the
    capacities --, text offsets, status, edit offsets)."""
    import torch

    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(lines)
    n = len(lines)
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_text = torch.full((capacity + 64,), 0x5A, dtype=torch.uint8, device=dev)
    d_edits = torch.full((edit_capacity * 24 + 48,), 0x5A, dtype=torch.uint8, device=dev)
    d_toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), 0x77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.normalize_aligned(d_utf8.data_ptr(), d_off.data_ptr(), n, d_text.data_ptr(), capacity, d_toff.data_ptr(), d_st.data_ptr(), d_edits.data_ptr(), edit_capacity,
                          d_eoff.data_ptr(), form)
    fits, nb, ne = ctx.try_sync_normalize_aligned()
    return (_lib.KGPU_OK if fits else _lib.KGPU_ERR_CAPACITY, nb, ne, d_text.cpu().numpy(), d_edits.cpu().numpy(), d_toff.cpu().numpy().view(np.uint64), d_st.cpu().numpy()[:n],
            d_eoff.cpu().numpy().view(np.uint64))


def test_capacity(env):
    from kanpyo_amd.device import DeviceContext

    lines = [("ﷺ" * 100).encode(), "ｶﾞＡＢＣ".encode(), b"", "東京".encode(), "ﾊﾝｶｸ㈱".encode()]
    want_text, want_off, want_status, want_edits, want_eoff = A.host_lines_aligned(lines, "NFKC")
    nb, ne = int(want_off[-1]), int(want_eoff[-1])
    assert nb > 3300 and ne == 100 + 4 + 5
    ctx = DeviceContext(env.tok)
    try:
        # the text fits and the edits do not; the edits fit and the text does not; one short of each; nothing at all
        for cap, ecap in ((nb, ne - 1), (nb - 1, ne), (nb - 1, ne - 1), (nb + 100, 0), (0, ne + 7), (0, 0)):
            rc, got, got_e, text, edits, toff, status, eoff = _device_run(ctx, lines, "NFKC", cap, ecap)
            assert (rc, got, got_e) == (_lib.KGPU_ERR_CAPACITY, nb, ne), (cap, ecap)
            assert (text == 0x5A).all() and (edits == 0x5A).all(), "a call that reports KGPU_ERR_CAPACITY wrote something"
        for cap, ecap in ((nb, ne), (nb + 37, ne + 5)):
            rc, got, got_e, text, edits, toff, status, eoff = _device_run(ctx, lines, "NFKC", cap, ecap)
            assert (rc, got, got_e) == (_lib.KGPU_OK, nb, ne)
            assert text[:nb].tobytes() == want_text.tobytes() and (text[nb:] == 0x5A).all()
            assert edits[: ne * 24].tobytes() == want_edits.tobytes() and (edits[ne * 24:] == 0x5A).all()
            assert np.array_equal(toff, want_off) and np.array_equal(status, want_status) and np.array_equal(eoff, want_eoff)
        # an unaligned normalise on the same context afterwards reports as it always did
        import torch

        from kanpyo_amd.tokenizer import pack_sentences

        utf8, offs = pack_sentences(lines)
        dev = torch.device("cuda", 0)
        d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_text = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
        d_toff = torch.zeros(len(lines) + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(len(lines), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.normalize(d_utf8.data_ptr(), d_off.data_ptr(), len(lines), d_text.data_ptr(), nb, d_toff.data_ptr(), d_st.data_ptr(), "NFKC")
        assert ctx.sync_normalize() == nb and d_text[:nb].cpu().numpy().tobytes() == want_text.tobytes()
        # the host form: the retry grows whichever was short; the raw call reports both
        text, toff, status, edits, eoff = env.tok.normalize_packed_aligned(utf8, offs)   # (first capacities 2 x and 1/4 x the input: the text is short)
        assert text.tobytes() == want_text.tobytes() and edits.tobytes() == want_edits.tobytes()
        out, ed = np.full(nb, 0x5A, dtype=np.uint8), np.full(ne * 24, 0x5A, dtype=np.uint8)
        got, got_e = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().kgpu_normalize_batch_aligned(env.tok.handle, 2, utf8.ctypes.data, offs.ctypes.data, len(lines), out.ctypes.data, nb, toff.ctypes.data, status.ctypes.data,
                                                     C.byref(got), ed.ctypes.data, ne - 1, eoff.ctypes.data, C.byref(got_e))
        assert rc == _lib.KGPU_ERR_CAPACITY and (got.value, got_e.value) == (nb, ne) and (out == 0x5A).all() and (ed == 0x5A).all()
    finally:
        ctx.close()


# ---- 5. spans, device against host -----------------------------------------------------------------------------------------------------------------------
def test_spans_of_a_real_tokenisation(env):
    from kanpyo_amd.tokenizer import pack_sentences

    rng = np.random.default_rng(43)
    keyed = ["ﾊﾝｶｸ", "ＡＢＣ", "㈱", "ｶﾞ", "東京", "１２３", "テスト", "辞書", "形態素"]   # what the dictionary's keys look like before NFKC: these lines tokenize whole
    lines = mixed_lines(300, seed=42) + ["".join(keyed[int(k)] for k in rng.integers(0, len(keyed), size=int(rng.integers(1, 30)))).encode() for _ in range(300)]
    lines += [s.encode() for s in SENTENCES[:10]]
    text, toff, status, edits, eoff = env.tok.normalize_packed_aligned(*pack_sentences(lines))
    tokens, koff, kstatus = env.tok.tokenize_packed(text, toff)
    assert len(tokens) > 1000 and len(edits) > 1000
    want = A.host_spans(tokens, koff, edits, eoff)
    got = env.tok.source_spans(tokens, koff, edits, eoff)
    assert got.dtype == A.SPAN_DTYPE and got.tobytes() == want.tobytes()
    # a slice of the batch: offsets that do not start at 0
    got = env.tok.source_spans(tokens, koff[100:400], edits, eoff[100:400])
    assert got.tobytes() == want[int(koff[100]) : int(koff[399])].tobytes()
    # what the spans mean: every token's source slice normalises to text that holds the token's surface
    raw, src = text.tobytes(), b"".join(lines)
    soff = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).tolist()
    k = koff.tolist()
    for i in (0, 5, 17, 300, len(lines) - 10, len(lines) - 7):
        for j in range(k[i], k[i + 1]):
            t, sp = tokens[j], want[j]
            if int(t["byte_len"]):
                a = soff[i] + int(sp["position"])
                surface = raw[int(toff[i]) + int(t["position"]) :][: int(t["byte_len"])]
                assert surface in N.host(src[a : a + int(sp["byte_len"])], "NFKC")[1]


CRAFT_LINES = {"none": "abcdefghij" * 20, "one": "x" * 100 + "Ａ" + "y" * 100, "many": "ｶﾞＡ㈱x" * 40}


def _craft(m, norm):
    """m records over the normalised line: m - 1 tokens of equal length (the last takes the rest) and the EOS dummy."""
    if m == 0:
        return []
    chars = len(norm)
    step = max(chars // max(m - 1, 1), 1)
    bounds = [min(i * step, chars) for i in range(m - 1)] + [chars]
    recs = [[len(norm[:a].encode()), len(norm[a:b].encode()), a, b] for a, b in zip(bounds, bounds[1:])]
    return recs + [[len(norm.encode()), 0, chars, chars + 3]]


def test_spans_of_crafted_records(env):
    sentences = []   # (records, edit tuples)
    for name, line in CRAFT_LINES.items():
        rc, out, _, _, ed, _ = A.host_aligned(line.encode(), "NFKC")
        assert rc == 0 and len(ed) == {"none": 0, "one": 1, "many": 120}[name]
        for m in (0, 1, 63, 64, 65, 130):   # the window edges of the records' walk
            recs = _craft(m, out.decode())
            assert len(recs) == m
            sentences.append((recs, ed))
    records = [r for recs, _ in sentences for r in recs]
    toff = np.concatenate([[0], np.cumsum([len(recs) for recs, _ in sentences])]).astype(np.uint64)
    eoff = np.concatenate([[0], np.cumsum([len(ed) for _, ed in sentences])]).astype(np.uint64)
    tokens, edits = A.token_array(records), A.edit_array([e for _, ed in sentences for e in ed])
    want = A.host_spans(tokens, toff, edits, eoff)
    assert A.span_lists(want) == [A.py_span(r, ed) for recs, ed in sentences for r in recs]
    got = env.tok.source_spans(tokens, toff, edits, eoff)
    assert got.tobytes() == want.tobytes()
    # a batch of sentences without records
    empty = env.tok.source_spans(tokens[:0], np.zeros(4, dtype=np.uint64), edits[:0], np.zeros(4, dtype=np.uint64))
    assert len(empty) == 0


def test_spans_of_arbitrary_records_touch_nothing_else(env):
    """Records of arbitrary values between two ordinary sentences: the call returns, and the neighbours' spans are right (rule 12: a record's fields are
    compared and added, never used as addresses)."""
    rng = np.random.default_rng(9)
    rc, out, _, _, ed, _ = A.host_aligned(CRAFT_LINES["many"].encode(), "NFKC")
    good = _craft(65, out.decode())
    junk = rng.integers(0, 1 << 32, size=(70, 4), dtype=np.uint64).tolist() + [[0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0xFFFFFFFF, 0, 0], [0xFFFFFFFF, 0, 7, 3]]
    tokens = A.token_array(good + junk + good)
    tokens["id"][len(good) : len(good) + len(junk)] = -5
    tokens["cls"][len(good) : len(good) + len(junk)] = 0xFFFFFFFF
    toff = np.array([0, len(good), len(good) + len(junk), 2 * len(good) + len(junk)], dtype=np.uint64)
    edits, eoff = A.edit_array(ed * 3), np.array([0, len(ed), 2 * len(ed), 3 * len(ed)], dtype=np.uint64)
    got = env.tok.source_spans(tokens, toff, edits, eoff)
    want = [A.py_span(r, ed) for r in good]
    assert len(got) == len(tokens) and A.span_lists(got[: len(good)]) == want and A.span_lists(got[len(good) + len(junk):]) == want


# ---- 6. the device-resident chain --------------------------------------------------------------------------------------------------------------------------
def test_device_chain(env):
    import torch

    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(SENTENCES)
    n, total = len(SENTENCES), int(offs[-1])
    want_text, want_off, want_status, want_edits, want_eoff = A.host_lines_aligned([s.encode() for s in SENTENCES], "NFKC")
    want_tokens, want_koff, want_kstatus = env.tok.tokenize_packed(want_text, want_off)
    want_spans = A.host_spans(want_tokens, want_koff, want_edits, want_eoff)
    assert len(want_edits) > 100 and len(want_tokens) > 100
    dev = torch.device("cuda", 0)
    d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    cap = 11 * total
    d_norm = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_noff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_nst = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_edits = torch.zeros(total * 24 + 24, dtype=torch.uint8, device=dev)
    d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ctx = DeviceContext(env.tok)
    try:
        torch.cuda.synchronize(dev)
        ctx.normalize_aligned(d_utf8.data_ptr(), d_off.data_ptr(), n, d_norm.data_ptr(), cap, d_noff.data_ptr(), d_nst.data_ptr(), d_edits.data_ptr(), total, d_eoff.data_ptr(), "NFKC")
        nbytes, nedits = ctx.sync_normalize_aligned()   # (the tokenizer's total_bytes and the buffers' sizes come from here)
        assert (nbytes, nedits) == (len(want_text), len(want_edits))
        tcap = nbytes + n + 64
        d_tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev)
        d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        d_spans = torch.full((tcap, 4), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.tokenize(d_norm.data_ptr(), d_noff.data_ptr(), n, nbytes, d_tok.data_ptr(), tcap, d_toff.data_ptr(), d_st.data_ptr())
        n_tok = ctx.sync()
        ctx.source_spans(d_tok.data_ptr(), d_toff.data_ptr(), n, d_edits.data_ptr(), d_eoff.data_ptr(), d_spans.data_ptr(), tcap)
        assert ctx.sync_lines() == 0
        assert n_tok == len(want_tokens) and np.array_equal(d_toff.cpu().numpy().view(np.uint64), want_koff)
        assert d_tok[:n_tok].cpu().numpy().tobytes() == want_tokens.tobytes()
        spans = d_spans.cpu().numpy()
        assert spans[:n_tok].tobytes() == want_spans.tobytes() and (spans[n_tok:] == -1).all()
        assert d_edits[: nedits * 24].cpu().numpy().tobytes() == want_edits.tobytes() and np.array_equal(d_eoff.cpu().numpy().view(np.uint64), want_eoff)
        # a span capacity below the token count: nothing at or behind it is stored
        d_spans.fill_(-1)
        torch.cuda.synchronize(dev)
        ctx.source_spans(d_tok.data_ptr(), d_toff.data_ptr(), n, d_edits.data_ptr(), d_eoff.data_ptr(), d_spans.data_ptr(), 70)
        ctx.sync_lines()
        spans = d_spans.cpu().numpy()
        assert spans[:70].tobytes() == want_spans[:70].tobytes() and (spans[70:] == -1).all()
    finally:
        ctx.close()


# ---- 7. tokenize_aligned end to end -----------------------------------------------------------------------------------------------------------------------
def test_tokenize_aligned(env):
    rows = env.tok.tokenize_aligned(["ﾊﾝｶｸＡＢＣ㈱", "テスト辞書", ""], normalize="NFKC")
    first = rows[0]
    assert [a.token.surface for a in first] == ["ハンカク", "ABC"] + [a.token.surface for a in first[2:-1]] + ["EOS"]
    assert "".join(a.token.surface for a in first[2:-1]) == "(株)" and len(first) >= 4
    assert [a.source_surface for a in first] == ["ﾊﾝｶｸ", "ＡＢＣ"] + ["㈱"] * (len(first) - 3) + ["EOS"]
    assert [(a.source_start, a.source_end) for a in first[:2]] == [(0, 4), (4, 7)] and all((a.source_start, a.source_end) == (7, 8) for a in first[2:-1])
    assert (first[-1].source_position, first[-1].source_byte_len, first[-1].source_start, first[-1].source_end) == (len("ﾊﾝｶｸＡＢＣ㈱".encode()), 0, 8, 11)
    assert [a.token for a in first] == env.tok.tokenize_batch(["ﾊﾝｶｸＡＢＣ㈱"], normalize="NFKC")[0]
    for row, plain in zip(rows[1:], env.tok.tokenize_batch(["テスト辞書", ""])):   # a clean line: the spans are the token's own fields
        assert [a.token for a in row] == plain
        for a in row:
            assert (a.source_position, a.source_start, a.source_end, a.source_surface) == (a.token.position, a.token.start, a.token.end, a.token.surface)
            assert a.source_byte_len == (0 if a.token.surface == "EOS" else len(a.token.surface.encode()))


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_align(env, tmp_path):
    from kanpyo_amd.dictfile import DictFile, save_dict

    path = tmp_path / "t.dict"
    save_dict(DictFile(env.dict, env.known, env.unk), str(path))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "align", "-c", str(path)], input="ﾊﾝｶｸＡＢＣ\nテスト辞書 \n\nｶﾞ東京\n".encode(), capture_output=True, env=envv, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == ("0\t4\tﾊﾝｶｸ\tハンカク\n4\t7\tＡＢＣ\tABC\nEOS\n" "0\t3\tテスト\tテスト\n3\t5\t辞書\t辞書\nEOS\n" "EOS\n" "0\t2\tｶﾞ\tガ\n2\t4\t東京\t東京\nEOS\n").encode()
