"""The device normaliser swept (kgpu_normalize.hip: classify, decode4, each_segment, the uploaded tables, the LDS column, the carried bases of the ALIGN
instantiation, the three branches of MODE_COPY): every scalar value, malformed UTF-8 at every unit and pass boundary, every source and destination
alignment, segments at the size limit, and lines of several passes.

The expected value is never the device's own output:
  text of a status-0 line   unicodedata.normalize of the whole line
  status 1                  exactly the lines Python's strict decoder rejects
  status 4                  the generator's reference (tools/gen_normalize_tables.py: normalize_line)
  edit records              align_ref.ref_edits (the generator's segments, each normalised by unicodedata); for the million-line batches the same records put
                            together with numpy from unicodedata's lengths and the generator's boundaries, and checked against ref_edits on a sample
  the host twin             kgpu_normalize_host_aligned agrees with all of the above wherever a batch is small enough to call it line by line
Every case runs through both instantiations (the plain call and the `_aligned` one) and, unless the case says otherwise, under NFC and NFKC.  No
tolerance: bytes, all n + 1 offsets, status bytes, edit records and edit offsets are compared exactly."""
import functools
import unicodedata

import numpy as np
import pytest

import align_ref as A
import normalize_ref as N
from kanpyo_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not N.versions_agree(), reason=f"Python's unicodedata is {unicodedata.unidata_version}, the committed tables are "
                                                  f"{_lib.lib().kgpu_normalize_unicode_version().decode()}")]

FORMS = ["NFC", "NFKC"]
KANA = "ｶﾞ"   # half-width ka + voiced mark: one segment, NFKC composes it
PASS, UNIT, MAX_SEGMENT = 1024, 16, 64


@pytest.fixture(scope="module")
def tok(fixture_dict):
    from kanpyo_amd import Tokenizer

    t = Tokenizer(fixture_dict)
    yield t
    t.close()


def device_both(tok, utf8, offs, form):
    """The batch through both instantiations -> ((text, offsets, status), (text, offsets, status, edits, edit offsets))."""
    return tok.normalize_packed(utf8, offs, form), tok.normalize_packed_aligned(utf8, offs, form)


def wrong_lines(got, want):
    """The lines at which a device result -- three arrays, or five -- is not `want` (five arrays): sorted indices."""
    n = len(want[2])
    if len(got[1]) != n + 1 or len(got[2]) != n or (len(got) == 5 and len(got[4]) != n + 1):
        return np.arange(n)
    bad = set(np.nonzero(got[2] != want[2])[0].tolist()) | set(N.differing_lines(got[0], got[1], want[0], want[1]).tolist())
    if len(got) == 5:
        bad |= set(A.differing_edit_lines(got[3], got[4], want[3], want[4]).tolist())
    # all n + 1 offsets, not only the lengths between them (offsets that differ behind a line of another length are that line's doing: it is counted alone)
    for k in (1, 4)[: 1 if len(got) == 3 else 2]:
        if not bad and not np.array_equal(got[k], want[k]):
            bad = set(np.nonzero(got[k][1:] != want[k][1:])[0].tolist()) | {0}
    return np.array(sorted(bad), dtype=np.int64)


def check_lines(tok, lines, form, want=None, host=True):
    """A list of lines through the device, both instantiations, against ref_edits (and the host twin against it too)."""
    from kanpyo_amd.tokenizer import pack_sentences

    want = A.expected_lines(lines, form) if want is None else want
    if host:
        twin = A.host_lines_aligned(lines, form)
        bad = wrong_lines(twin, want)
        assert bad.size == 0, f"{form}: the host twin differs from the reference at {bad.size} lines, first {[bytes(lines[i])[:40].hex() for i in bad[:4]]}"
    utf8, offs = pack_sentences(lines)
    for name, got in zip(("plain", "aligned"), device_both(tok, utf8, offs, form)):
        bad = wrong_lines(got, want)
        if bad.size:
            i = int(bad[0])
            pytest.fail(f"{form} {name}: {bad.size} of {len(lines)} lines differ, first at {bad[:8].tolist()}: line {i} is {len(lines[i])} bytes, begins {bytes(lines[i])[:24].hex()}, "
                        f"ends {bytes(lines[i])[-24:].hex()}, status {int(got[2][i])} for {int(want[2][i])}")
    return want


# ---- 1. every scalar value through the device tables ---------------------------------------------------------------------------------------------------
# (a) alone: the line's first code point and its last -- the single-inert fast path with nothing behind it, or a walk of one code point
# (b) marks: every starter is walked, composed with U+0301 and reordered around U+0323; the line is ONE segment (neither mark has a boundary before it)
# (c) straddle: behind thirteen ASCII bytes a 3- or 4-byte code point crosses the first unit boundary of a 16-aligned line, and the lead byte of the
#     half-width ka behind it falls in bits 16 .. 19 of the unit's masks
# (d) behind: a segment that changes (e + acute) stands in front.  The text does not show whether c's boundary bit is right -- a code point that
#     neither decomposes nor composes comes out the same inside the segment in front as in one of its own --; where that segment's edit record ends does.
CONTEXTS = {"alone": ("", ""), "marks": ("", "\u0301\u0323"), "straddle": ("x" * 13, KANA), "behind": ("e\u0301", "q")}


@functools.lru_cache(maxsize=None)
def alone_reference(form):
    """unicodedata of every scalar value as a line of its own -> (bytes, code points, changed) per code point."""
    _, _, out_bytes, out_chars, changed = N.normalize_strings([chr(c) for c in N.scalars().tolist()], form)
    return out_bytes, out_chars, changed


def _fixed_segments(text, form):
    """The edit records of a piece that stands by itself, and its four lengths (output bytes, source bytes, output and source code points): ref_edits' sums."""
    edits, op, sp, oc, sc = [], 0, 0, 0, 0
    for seg in N.GEN.segments(text, form):
        norm = unicodedata.normalize(form, seg)
        s, n = seg.encode(), norm.encode()
        if s != n:
            edits.append((op, sp, oc, sc, len(n), len(s), len(norm), len(seg)))
        op, sp, oc, sc = op + len(n), sp + len(s), oc + len(norm), sc + len(seg)
    assert A.ref_edits(text.encode(), form) == (unicodedata.normalize(form, text).encode(), 0, edits)
    return edits, (op, sp, oc, sc)


def scalar_sweep_reference(context, form):
    """-> (utf8, offsets, the five expected arrays) for the batch of all scalar values in the context: one line per code point, in the order of scalars()."""
    pre, suf = CONTEXTS[context]
    cps = N.scalars()
    n = cps.size
    strs = [pre + chr(c) + suf for c in cps.tolist()]
    cp_bytes = N.utf8_len(cps)
    utf8, offs = N.pack_strings(strs, cp_bytes + len(pre.encode()) + len(suf.encode()))
    text, toff, out_bytes, out_chars, changed = N.normalize_strings(strs, form)
    src_bytes = np.diff(offs.astype(np.int64))
    zero = np.zeros(n, dtype=np.int64)
    if context in ("alone", "marks"):   # one segment per line: an edit exactly where the bytes change
        gen = N.GEN
        assert not gen.boundary_before(0x0301, form) and not gen.boundary_before(0x0323, form)
        m = changed
        counts = m.astype(np.int64)
        edits = A.edit_columns(out_pos=zero[m], src_pos=zero[m], out_char=zero[m], src_char=zero[m], out_len=out_bytes[m], src_len=src_bytes[m], out_chars=out_chars[m],
                               src_chars=np.full(int(m.sum()), 1 + len(suf)))
        eoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    else:
        # Where c has a boundary before it the line's segments are those of the prefix (each with the result it has by itself), c (its result is the "alone"
        # line's) and those of the suffix.  Where it has none (a mark, a jamo vowel, a second member of a pair: a thousand code points) it joins the
        # segment in front: ref_edits, line by line.
        gen = N.GEN
        assert gen.boundary_before(ord(suf[0]), form)
        B = N.boundary_table(form)
        assert 500 < int((~B).sum()) < 5000
        one_bytes, one_chars, one_changed = alone_reference(form)
        pre_edits, (p_ob, p_sb, p_oc, p_sc) = _fixed_segments(pre, form)
        suf_edits, (s_ob, _, s_oc, _) = _fixed_segments(suf, form)
        assert p_sb == len(pre.encode()) and p_sc == len(pre)
        # (what the concatenation of the segments gives is what unicodedata gives for the whole line)
        assert np.array_equal(out_bytes[B], p_ob + one_bytes[B] + s_ob) and np.array_equal(out_chars[B], p_oc + one_chars[B] + s_oc)
        counts = np.where(B, len(pre_edits) + one_changed.astype(np.int64) + len(suf_edits), 0)
        slow = {int(i): A.ref_edits(strs[i].encode(), form)[2] for i in np.nonzero(~B)[0]}
        for i, ed in slow.items():
            counts[i] = len(ed)
        eoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        edits = np.zeros(int(eoff[-1]), dtype=A.EDIT_DTYPE)
        at = eoff[:-1].astype(np.int64)
        for j, e in enumerate(pre_edits):
            edits[at[B] + j] = A.edit_array([e])[0]
        m = B & one_changed
        edits[at[m] + len(pre_edits)] = A.edit_columns(out_pos=zero[m] + p_ob, src_pos=zero[m] + p_sb, out_char=zero[m] + p_oc, src_char=zero[m] + p_sc, out_len=one_bytes[m],
                                                       src_len=cp_bytes[m], out_chars=one_chars[m], src_chars=zero[m] + 1)
        for j, e in enumerate(suf_edits):   # (the suffix's records, moved behind the prefix and c)
            edits[at[B] + len(pre_edits) + one_changed[B] + j] = A.edit_columns(
                out_pos=p_ob + one_bytes[B] + e[0], src_pos=p_sb + cp_bytes[B] + e[1], out_char=p_oc + one_chars[B] + e[2], src_char=zero[B] + p_sc + 1 + e[3],
                out_len=zero[B] + e[4], src_len=zero[B] + e[5], out_chars=zero[B] + e[6], src_chars=zero[B] + e[7])
        for i, ed in slow.items():
            edits[int(eoff[i]) : int(eoff[i + 1])] = A.edit_array(ed)
    # the records put together above are ref_edits' own on a sample: every 1021st code point and the awkward pool
    index = {int(c): i for i, c in enumerate(cps.tolist())}
    for i in sorted(set(range(0, n, 1021)) | {index[c] for c in N.AWKWARD}):
        out, status, ed = A.ref_edits(strs[i].encode(), form)
        assert status == 0 and A.edit_tuples(edits[int(eoff[i]) : int(eoff[i + 1])]) == ed and out == text[int(toff[i]) : int(toff[i + 1])].tobytes(), hex(int(cps[i]))
    return utf8, offs, (text, toff, np.zeros(n, dtype=np.uint8), edits, eoff)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("context", list(CONTEXTS))
def test_every_scalar_value(tok, context, form):
    """All 1 112 064 scalar values, one per line, in one batch: 135 times as many lines as the launch has workgroups."""
    utf8, offs, want = scalar_sweep_reference(context, form)
    cps = N.scalars()
    assert len(want[2]) == cps.size == 1112064 and cps.size > 100 * 8192
    for name, got in zip(("plain", "aligned"), device_both(tok, utf8, offs, form)):
        bad = wrong_lines(got, want)
        if bad.size:
            pytest.fail(f"{form} {context} {name}: {bad.size} code points differ, first {[hex(int(c)) for c in cps[bad[:8]]]}")


@pytest.mark.parametrize("form", FORMS)
def test_every_composition_pair(tok, form):
    """The device's copy of comp_key / comp_val at every entry: each pair alone, behind a starter, and its composite (the strings of the CPU sweep)."""
    pairs, _ = N.GEN.pairs_and_seconds()
    strings = [chr(a) + chr(b) for a, b in pairs] + ["a" + chr(a) + chr(b) for a, b in pairs] + [chr(c) for c in pairs.values()]
    lines = [s.encode() for s in strings]
    want = A.expected_lines(lines, form)
    assert not want[2].any() and len(pairs) > 900 and len(want[3]) > 900
    check_lines(tok, lines, form, want)


# ---- 2. malformed UTF-8 against the strict decoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pad", [0, 15])
def test_every_two_byte_string(tok, form, pad):
    """All 65 536 two-byte strings as a whole line, and behind fifteen ASCII bytes (on a 16-aligned line the pair is split across two units)."""
    lines = [b"p" * pad + bytes([a, b]) for a in range(256) for b in range(256)]
    want = A.expected_lines(lines, form, unchanged_has_none=True)
    ok = np.array([N.strict_utf8(ln) for ln in lines])
    assert np.array_equal(want[2] == 0, ok) and int(ok.sum()) == 128 * 128 + 30 * 64   # ASCII pairs and the two-byte sequences C2 .. DF + 80 .. BF
    check_lines(tok, lines, form, want)


MALFORMED = [bytes.fromhex(h) for h in (
    "80", "bf", "c0af", "c1bf", "e080af", "e09fbf", "eda080", "edbfbf", "f0808080", "f08fbfbf", "f4908080",
    "f5", "f6", "f7", "f8", "f9", "fa", "fb", "fc", "fd", "fe", "ff",
    "c241", "e341", "e38141", "f041", "f09041", "f0908041",                 # a lead byte (and some of its continuation bytes) followed by ASCII
    "c2c280", "e3e38182", "e381e38182", "f0f0908080", "f09080f0908080", "dfe0a080",   # ... followed by another lead
    "f090808080", "f48fbfbf80", "e3818280", "c28080",                       # a valid sequence and one more continuation byte
    "c2", "df", "e3", "e381", "ef", "efbf", "f0", "f090", "f09080", "f4", "f48f", "f48fbf",   # every proper prefix of a valid sequence (at the line's end)
)]
EXTREMES = [bytes.fromhex(h) for h in ("c280", "dfbf", "e0a080", "ed9fbf", "ee8080", "efbfbf", "f0908080", "f48fbfbf")]
MALFORMED_PADS = list(range(0, 20)) + list(range(1005, 1028))


def test_the_listed_classes_are_what_they_claim():
    assert all(not N.strict_utf8(m) for m in MALFORMED) and all(N.strict_utf8(e) for e in EXTREMES)
    assert [ord(e.decode()) for e in EXTREMES] == [0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("around", ["bare", "between"])
def test_malformed_at_every_boundary(tok, form, around):
    """Each class of malformed sequence and each valid extreme behind every ASCII pad of 0 .. 19 and 1005 .. 1027 bytes -- wherever the packing puts the
    line, the piece meets every byte of a unit and the pass boundary --: with nothing behind it, and with the kana pair in front and a q behind."""
    front, back = (b"", b"") if around == "bare" else (KANA.encode(), b"q")
    lines = [front + b"p" * pad + piece + back for piece in MALFORMED + EXTREMES for pad in MALFORMED_PADS]
    want = A.expected_lines(lines, form)
    n_bad = len(MALFORMED) * len(MALFORMED_PADS)
    assert (want[2][:n_bad] == 1).all() and not want[2][n_bad:].any() and np.array_equal(want[2] == 0, [N.strict_utf8(ln) for ln in lines])
    e = want[4].astype(np.int64)
    assert (np.diff(e)[:n_bad] == 0).all() and (form == "NFC" or around == "bare" or (np.diff(e)[n_bad:] >= 1).all())   # an invalid line has no edits, dirty or not
    check_lines(tok, lines, form, want)


@pytest.mark.parametrize("form", FORMS)
def test_a_sequence_split_across_two_lines(tok, form):
    """Line i ends with the first bytes of a sequence and line i + 1 begins with the rest: in the packed buffer the bytes are a valid sequence, and both
    lines are status 1 -- every split point of a 3-byte and a 4-byte sequence, inside the batch and with line i + 1 the batch's last."""
    pairs = [(seq[:k], seq[k:]) for seq in ("あ".encode(), "😀".encode()) for k in range(1, len(seq))]
    assert len(pairs) == 5 and pairs[1] == (b"\xe3\x81", b"\x82")
    body = []
    for head, tail in pairs:
        for pad in (0, 3, 13, 14, 15, 16, 1021, 1022, 1023):   # the cut at a unit and at a pass boundary of the buffer as well
            body += [b"p" * pad + head, tail + b"q" * (pad % 5), KANA.encode()]
    for head, tail in pairs:
        lines = body + [b"ok", head, tail]
        want = check_lines(tok, lines, form)
        assert want[2][-2:].tolist() == [1, 1] and want[2][-3] == 0 and want[2][:-3].tolist() == [1, 1, 0] * (len(body) // 3)
        assert want[0][int(want[1][-3]):].tobytes() == head + tail


# ---- 3. every source and destination alignment -----------------------------------------------------------------------------------------------------------
def _ascii(n, salt):
    """n ASCII bytes that differ from place to place (a copy that lands a few bytes off shows)."""
    return bytes(0x21 + (7 * j + 3 * salt + j // 11) % 94 for j in range(n))


COPY_LENGTHS = list(range(0, 41)) + [63, 64, 65, 1023, 1024, 1025]


@functools.lru_cache(maxsize=None)
def alignment_batch(form):
    """-> (lines, copied[bool]: the lines MODE_COPY takes -- ASCII alone, or not UTF-8 --, the expected arrays)."""
    lines, copied = [], []
    for n in COPY_LENGTHS:   # clean: the head, the full units and the tail of each copy branch
        lines.append(_ascii(n, n))
        copied.append(True)
    for n in COPY_LENGTHS[1:]:   # not UTF-8: copied too
        ln = bytearray(_ascii(n, n + 1))
        ln[n // 2] = 0xFF
        lines.append(bytes(ln))
        copied.append(True)
    for seg in ("µ", KANA, "\U0001d15e", "😀\u0301"):   # one dirty segment behind every pad
        for pad in range(0, 34):
            lines.append(_ascii(pad, pad) + seg.encode())
            copied.append(False)
    # lines that shrink (e + acute: 3 -> 2 bytes under both forms) and grow (U+0958: 3 -> 6; U+FDFA under NFKC: 3 -> 33), and copied lines behind each
    for grow in ("\u0958", "ﷺ", "\u0958\u0958"):
        lines += [grow.encode() + b"z", _ascii(50, 5)]
        copied += [False, True]
    for j in range(16):   # one byte less in front of each group: the copied lines meet every dmis - mis
        lines += ["e\u0301".encode(), _ascii(70 + j, j), _ascii(9, j)[:4] + b"\xc0" + _ascii(80, j), _ascii(1030, j)]
        copied += [False, True, True, True]
    lines.append((KANA + "x").encode() + b"\xff" + KANA.encode())   # not UTF-8 AND dirty: as it is
    copied.append(True)
    want = A.expected_lines(lines, form)
    twin = A.host_lines_aligned(lines, form)
    assert wrong_lines(twin, want).size == 0
    return lines, np.array(copied), want


def _copy_parts(mis, dmis, n):
    """The parts of k_norm_write's MODE_COPY that a line of n bytes at these two misalignments runs: (branch, part) pairs."""
    if dmis == mis:
        branch, unit, to_boundary = "units", 16, (16 - dmis) & 15
    elif (dmis ^ mis) & 3 == 0:
        branch, unit, to_boundary = "words", 4, (4 - (dmis & 3)) & 3
    else:
        return {("bytes", "all")} if n else set()
    head = min(to_boundary, n)
    full = (n - head) // unit
    return {(branch, part) for part, there in (("head", head), ("full", full), ("tail", n - head - unit * full)) if there}


@pytest.mark.parametrize("form", FORMS)
def test_every_alignment(tok, form):
    """The device form over torch tensors, the source at d_utf8[b:] for every b of 0 .. 15 and the destination at d_text[c:] with (c - b) mod 16 of 0, 4
    and 1: the test sets the address bits itself and asserts which misalignments and copy branches the batch reached."""
    import torch

    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    lines, copied, want = alignment_batch(form)
    want_text, want_off, want_status, want_edits, want_eoff = want
    utf8, offs = pack_sentences(lines)
    n, total, n_edits = len(lines), int(want_off[-1]), int(want_eoff[-1])
    cap, ecap = total + 37, n_edits + 5
    lens = np.diff(offs.astype(np.int64))
    assert n_edits > 50 and set(np.diff(want_off.astype(np.int64)) - lens) >= {-1, 3}
    dev = torch.device("cuda", 0)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    reached, seen_mis = set(), set()
    ctx = DeviceContext(tok)
    try:
        for b in range(16):
            # (a lead byte in front of the first line and continuation bytes behind the last: nothing outside a line may be looked at)
            d_src = torch.from_numpy(np.concatenate([np.full(b, 0xE3, dtype=np.uint8), utf8, np.full(16, 0x80, dtype=np.uint8)])).to(dev)
            for delta in (0, 4, 1):
                c = (b + delta) % 16
                for aligned in (False, True):
                    d_text = torch.full((c + cap + 64,), 0x5A, dtype=torch.uint8, device=dev)
                    d_toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                    d_st = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
                    d_edits = torch.full((ecap * 24 + 48,), 0x5A, dtype=torch.uint8, device=dev)
                    d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize(dev)
                    src, dst = d_src.data_ptr() + b, d_text.data_ptr() + c
                    if aligned:
                        ctx.normalize_aligned(src, d_off.data_ptr(), n, dst, cap, d_toff.data_ptr(), d_st.data_ptr(), d_edits.data_ptr(), ecap, d_eoff.data_ptr(), form)
                        assert ctx.sync_normalize_aligned() == (total, n_edits)
                    else:
                        ctx.normalize(src, d_off.data_ptr(), n, dst, cap, d_toff.data_ptr(), d_st.data_ptr(), form)
                        assert ctx.sync_normalize() == total
                    text = d_text.cpu().numpy()
                    got = (text[c : c + total], d_toff.cpu().numpy().view(np.uint64), d_st.cpu().numpy())
                    if aligned:
                        raw = d_edits.cpu().numpy()
                        got += (raw[: n_edits * 24].view(A.EDIT_DTYPE), d_eoff.cpu().numpy().view(np.uint64))
                        assert (raw[n_edits * 24:] == 0x5A).all(), "edit records behind the reported number"
                    bad = wrong_lines(got, want)
                    assert bad.size == 0, f"{form} b={b} c={c} aligned={aligned}: {bad.size} lines differ, first {bad[:8].tolist()} ({[lines[i][:20].hex() for i in bad[:3]]})"
                    assert (text[:c] == 0x5A).all() and (text[c + total:] == 0x5A).all(), f"{form} b={b} c={c} aligned={aligned}: bytes outside the text were written"
                    # what this run covered, from the addresses themselves
                    mis = (src + offs[:-1].astype(np.int64)) & 15
                    dmis = (dst + want_off[:-1].astype(np.int64)) & 15
                    assert set(mis.tolist()) == set(range(16)) and set(mis[copied].tolist()) == set(range(16))
                    assert set(((dmis - mis) & 15)[copied].tolist()) == set(range(16))   # behind the shrinking lines: every dmis - mis
                    parts = set()
                    for i in np.nonzero(copied)[0]:
                        parts |= _copy_parts(int(mis[i]), int(dmis[i]), int(lens[i]))
                    first = {0: "units", 4: "words", 1: "bytes"}[delta]   # the branch of the lines in front of the first one that shrinks
                    assert _copy_parts(int(mis[0]), int(dmis[0]), 1).pop()[0] == first and {p for p in parts if p[0] == first} >= ({(first, "all")} if first == "bytes" else {(first, "head"), (first, "full"), (first, "tail")})
                    reached |= {(delta, aligned) + p for p in parts}
                    seen_mis |= {(b, int(m)) for m in mis}
    finally:
        ctx.close()
    everything = {("units", "head"), ("units", "full"), ("units", "tail"), ("words", "head"), ("words", "full"), ("words", "tail"), ("bytes", "all")}
    for delta in (0, 4, 1):
        for aligned in (False, True):
            assert {p[2:] for p in reached if p[:2] == (delta, aligned)} == everything
    assert len(seen_mis) == 256


# ---- 4. the segment limit, on and off a pass boundary ------------------------------------------------------------------------------------------------------
MARK = "\u0301"
LIMIT_PIECES = [   # (what stands around the marks, marks at the limit, forms)
    (("a", ""), 64, FORMS), (("a", "\u0344"), 62, FORMS), (("각", ""), 62, FORMS), (("\U0001d15e", ""), 63, FORMS), (("\U0001d160", ""), 62, FORMS), (("ﷺ", ""), 47, ["NFKC"]),
]
LIMIT_PADS = [0, 15, 16] + list(range(1000, 1025))


def _piece(around, marks):
    return around[0] + MARK * marks + around[1]


@pytest.mark.parametrize("form", FORMS)
def test_segment_limit(tok, form):
    """Segments of exactly KGPU_NORMALIZE_MAX_SEGMENT + 1 code points after decomposition (status 0) and of one more (status 4), and the insertion sort at full
    length, behind pads that put the walk across the pass boundary."""
    pieces = [(_piece(around, m), 0) for around, m, forms in LIMIT_PIECES if form in forms] + [(_piece(around, m + 1), 4) for around, m, forms in LIMIT_PIECES if form in forms]
    pieces.append(("a" + "\u0301\u0323" * 32, 0))   # 32 marks of class 230 each in front of one of class 220: the sort moves every second entry
    for piece, status in pieces:   # the generator's reference confirms every row, and the pieces sit AT the limit
        deco = len(unicodedata.normalize(N.GEN.FORMS[form], piece))
        assert N.GEN.normalize_line(piece.encode(), form)[1] == status and deco == (MAX_SEGMENT + 1 if status == 0 else MAX_SEGMENT + 2), (piece[:2], deco)
        assert len(list(N.GEN.segments(piece, form))) == 1
    lines, expect = [], []
    for piece, status in pieces:
        for pad in LIMIT_PADS:
            lines += [b"p" * pad + piece.encode(), b"p" * pad + piece.encode() + "q東".encode()]
            expect += [status, status]
    over = _piece(("a", ""), 65)
    lines += [(KANA + "e\u0301" + over + KANA).encode(), (over + "e\u0301").encode(), ("\u0958x" * 40 + over).encode()]   # a status-4 piece beside dirty segments: unchanged, no edits
    expect += [4, 4, 4]
    want = check_lines(tok, lines, form)
    assert want[2].tolist() == expect
    e, o = want[4].astype(np.int64), want[1].astype(np.int64)
    for i, ln in enumerate(lines):   # a status-4 line: unchanged and without edits; any other has edits exactly when its bytes change
        assert (e[i] == e[i + 1]) == (want[0][o[i] : o[i + 1]].tobytes() == ln) and (not expect[i] or e[i] == e[i + 1])


# ---- 5. long random lines ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_lines():
    strings = N.random_strings(20261019, 30000)
    rng = np.random.default_rng(5)
    lines, i = [], 0
    while i < len(strings):
        k = int(rng.integers(1, 121))
        lines.append("".join(strings[i : i + k]).encode())
        i += k
    return lines


@pytest.mark.parametrize("form", FORMS)
def test_long_random_lines(tok, form):
    """Lines of up to 120 random strings from the awkward pool: most are longer than one pass, a tenth longer than two."""
    lines = long_lines()
    sizes = np.array([len(ln) for ln in lines])
    assert 2 * int((sizes > PASS).sum()) > len(lines) and int((sizes > 2 * PASS).sum()) > 30 and len(lines) > 400
    want = A.expected_lines(lines, form)
    assert not want[2].any(), "a line the reference leaves unnormalised would hide what the device does with it"
    assert want[0].tobytes() == b"".join(unicodedata.normalize(form, ln.decode()).encode() for ln in lines) and len(want[3]) > 10000
    check_lines(tok, lines, form, want)
