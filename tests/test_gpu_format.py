"""The line renderer alone (kgpu_format.hip behind kgpu_format_lines_device / kgpu_ctx_sync_lines) on crafted records: every destination
misalignment, window edges at chosen places, more sentences than one trip of the grid, output past 4 GiB, bad records late in the work, and
the protocol around the report words.  Every test builds its input in numpy, uploads it with torch, renders on a context that has never
tokenized and compares d_text[:total] and all n + 1 text offsets byte for byte with tests/lines_ref.py::render (pinned on the CPU by
tests/test_lines_ref_cpu.py).  No tolerance.  Every destination has 0xAB margins of 64 bytes or more on both sides, and the words around the
offsets are canaries too; they and d_text[total:] must come back untouched."""
import numpy as np
import pytest

import lines_ref as R
from conftest import fixture_dict_parts
from record_cases import FILL, _Dest, _enqueue, _Input, _sync

pytestmark = pytest.mark.gpu


# ---- dictionaries and contexts ----------------------------------------------------------------------------------------------------------
class _Dict:
    def __init__(self, tok, known, unk):
        from kanpyo_amd.device import DeviceContext

        info = tok.info()
        self.tok, self.nk, self.nu = tok, info["n_morphs"], info["n_unk_morphs"]
        self.krows, self.urows = R.rows_of(known, self.nk), R.rows_of(unk, self.nu)
        self.ctx = DeviceContext(tok)   # never tokenizes: kgpu_format_lines_device asks only that no tokenize batch is pending

    def render(self, case):
        return R.render(*case, self.krows, self.urows)


@pytest.fixture(scope="module")
def small():
    """The small dictionary of test_gpu_lines.py::test_edge_cases: known rows of 0, 62 and 10 200 bytes, an unknown row, an empty-string name."""
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.dictfile import MorphFeatureTable

    p = fixture_dict_parts()
    p["conn_data"] = [0, 100, 200, 100, -30000, 100, 200, 100, -30000]
    p["morphs"] = [[0, 0, 1000], [1, 1, -20000], [2, 2, 1100]]
    k = MorphFeatureTable([[], [1, 0, 1], [2]], ["", "名" * 10, "長" * 3400])
    u = MorphFeatureTable([[1]] * len(p["unk_morphs"]), ["", "未知"])
    tok = Tokenizer(Dict.from_parts(**p))
    tok.set_features(k, u)
    d = _Dict(tok, k, u)
    assert [len(r) for r in d.krows] == [0, 62, 10200] and d.urows[0] == "未知".encode()
    yield d
    d.ctx.close()


@pytest.fixture(scope="module")
def synth_d():
    """synth.build_dict() with synth.feature_tables: realistic row lengths, hundreds of thousands of ids."""
    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    d = _Dict(tok, known, unk)
    assert d.nk > 100_000
    yield d
    d.ctx.close()


# ---- render, compare ---------------------------------------------------------------------------------------------------------------------
def _check(d, inp, want, want_off, mis, slack=32):
    from kanpyo_amd import _lib

    dest = _Dest(inp.n, len(want) + slack, mis)
    _enqueue(d.ctx, inp, dest)
    assert _sync(d.ctx) == (_lib.KGPU_OK, len(want))
    dest.holds(want, want_off)


def _check_all_mis(d, case, mis_set):
    want, want_off = d.render(case)
    inp = _Input(case)
    for mis in mis_set:
        try:
            _check(d, inp, want, want_off, mis)
        except AssertionError as e:
            raise AssertionError(f"mis {mis}, n {inp.n}, {inp.T} records, {len(want)} bytes: {e}") from None
    return want, want_off


# ---- 1. every alignment x every small size ------------------------------------------------------------------------------------------------
def _sized_case(rng, size):
    """One sentence whose handful of short lines render to exactly `size` bytes (small dictionary): id-0 records, EOS, the unknown row, the
    0-byte and 62-byte known rows."""
    text = rng.integers(0, 256, size=96, dtype=np.uint8).tobytes()
    recs, left = [], size
    while left:
        L = left if len(recs) == 4 or left < 4 else int(rng.integers(2, left + 1))
        if left - L == 1:
            L = left
        shapes = [(0, R.KNOWN, 2), (1, R.KNOWN, 2)]   # (id, class, bytes of the line besides the surface)
        if L >= 8:
            shapes.append((1, R.UNKNOWN, 8))
        if L >= 64:
            shapes.append((2, R.KNOWN, 64))
        tid, cls, fixed = shapes[int(rng.integers(0, len(shapes)))]
        if L == 5 and rng.integers(0, 2):
            recs.append((0, R.DUMMY, 0, 0))
        else:
            recs.append((tid, cls, int(rng.integers(0, 96 - (L - fixed) + 1)), L - fixed))
        left -= L
    return R.pack([text], [recs])


def test_every_alignment_every_size_to_80(small):
    """One sentence of every total size from 0 to 80 bytes (1 excepted: a line has two bytes or more) at each of the sixteen misalignments:
    below one unit, exactly one unit, a head and a tail only, and so on."""
    rng = np.random.default_rng(1)
    for size in [0] + list(range(2, 81)):
        for rep in range(2):
            case = _sized_case(rng, size)
            want, _ = _check_all_mis(small, case, range(16))
            assert len(want) == size
    # no sentence at all, and sentences without records
    _check_all_mis(small, R.pack([], []), range(16))
    _check_all_mis(small, R.pack([b"abc", b"", b"d"], [[], [], []]), range(16))


@pytest.mark.parametrize("which", ["small", "synth"])
def test_every_alignment_random_small_batches(small, synth_d, which):
    d = small if which == "small" else synth_d
    rng = np.random.default_rng(2 if which == "small" else 3)
    ids = [1] * 6 + [2] * 6 + [3] if which == "small" else None
    for i in range(150):
        case = R.make_records(rng, int(rng.integers(1, 13)), (0, 4), R.KINDS, d.nk, d.nu, known_ids=ids)
        _check_all_mis(d, case, range(16))


# ---- 2. window edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["two", "cycle", "big"])
def test_window_edges(small, regime):
    """One sentence of 0 .. 1000 records, rendered 64 at a time, at misalignments 0, 1, 9 and 15.  'two': eight line starts share a unit.
    'cycle': line lengths 2..40, so that over the set the first byte of a later window falls on every offset 0..15 of a unit (asserted from
    the reference's own line lengths).  'big': lines of 10 203 bytes and more between two-byte lines: a line spans several 1024-byte passes of
    the wavefront and ends mid-unit."""
    seen = set()
    for T in R.WINDOW_TOKENS:
        case = R.window_case(regime, T)
        _check_all_mis(small, case, R.WINDOW_MIS)
        starts = np.concatenate([[0], np.cumsum(R.line_lengths(*case, small.krows, small.urows))])[64:T:64]
        seen |= {int(s + mis) % 16 for s in starts for mis in R.WINDOW_MIS}
    if regime == "cycle":
        assert seen == set(range(16)), f"window starts fell on offsets {sorted(seen)} only"


# ---- 3. many sentences --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.MANY_N)
def test_many_sentences(synth_d, n):
    """Across k_lines_scan's 256/1024-thread switch (n > 256), its carry over several rounds (n > 1024) and the second and third trip of the
    grid-stride loops (n > 32 768, n > 65 536): 0-3 short records per sentence, half of the sentences without any.  At 70 001 a sentence of
    200 records sits at index 0, at 32 768 and at 70 000."""
    rng = np.random.default_rng(n)
    case = R.many_case(rng, n, synth_d.nk, synth_d.nu, long_at=(0, 32768, 70000) if n == 70001 else ())
    _check_all_mis(synth_d, case, (0, 5))


# ---- 4. past 4 GiB ------------------------------------------------------------------------------------------------------------------------
def test_output_past_4gib(small):
    """512 sentences, 460 800 records naming the 10 200-byte row, lines of 10 203 bytes: 4 701 542 400 bytes (>= 2^32 + 2^28) at a destination
    misaligned by 7, checked on the device without a 4 GiB host copy: the offsets against the numpy running sum, and d_text[:total] as a
    [T, 10203] matrix -- column 0 the expected surface bytes, column 1 the tab, columns 2..10201 the row, the last column the newline.

    The records are not spread evenly (900 per sentence on average): sentences 64..95 have 13 800 each, the others 40.  k_lines_scan scans 64
    sentences per wavefront with wave_incl_scan64 and adds the wavefronts' sums in plain 64-bit arithmetic, and a step of that scan adds what a
    lower lane hands up to a lane's own 64-bit value.  The high word that crosses lanes therefore matters only where the partial sum of at most
    32 neighbouring lanes of ONE wavefront passes 2^32.  With an even 880 records per sentence a wavefront's 64 lengths sum to 575 MB, and a
    scan that handed up the low word alone passes (tried: it also passed with 6900 records in each of sentences 64..127, where lanes 0..31 and
    32..63 hold 2.25 GB each).  Here lanes 0..31 of the second wavefront hold more than 2^32 bytes together (asserted below), which lane 31 hands
    to lane 63 in the scan's last step, and one of those sentences straddles byte 2^32.
    Out of scope: a single sentence past 4 GiB (420 000 records in one sentence).
    Wall time on an MI355X (pytest --durations, whole GPU suite in one run): 0.65 s, next to 16.9 s for the slowest test of test_gpu_split.py
    (test_cli_split_device_writes_what_the_default_writes) and 15.2 s for its test_large_block_64_mib; this whole file takes 13 s, 5.6 s of it
    building the synthetic dictionary."""
    import torch

    from kanpyo_amd import _lib

    counts = np.full(512, 40, dtype=np.int64)
    counts[64:96] = 13800
    rng = np.random.default_rng(4)
    case = R.big_case(rng, counts)
    utf8, offsets, tokens, tok_offsets = case
    T, W = int(counts.sum()), 10203
    total = T * W
    want_off = np.concatenate([[0], np.cumsum(counts * W)]).astype(np.uint64)
    assert total >= 2**32 + 2**28
    assert ((want_off[:-1] < 2**32) & (want_off[1:] > 2**32)).any(), "no sentence straddles byte 2^32"
    assert int((counts[64:96] * W).sum()) > 2**32, "no partial sum that crosses lanes in the scan passes 2^32"
    inp = _Input(case)
    dest = _Dest(inp.n, total + 32, 7)
    _enqueue(small.ctx, inp, dest)
    assert _sync(small.ctx) == (_lib.KGPU_OK, total)
    assert np.array_equal(dest.offsets(), want_off)
    dev = dest.buf.device
    text = dest.buf[dest.lead : dest.lead + total].view(T, W)
    sent = np.repeat(np.arange(512), counts)
    idx = np.arange(T) - np.repeat(tok_offsets[:-1].astype(np.int64), counts)
    col0 = torch.from_numpy(utf8[sent * 251 + idx % 251].copy()).to(dev)
    bad = torch.nonzero(text[:, 0] != col0)
    assert bad.numel() == 0, f"{bad.numel()} lines start with another surface byte, the first is line {int(bad[0])}"
    assert bool((text[:, 1] == 9).all()) and bool((text[:, W - 1] == 10).all())
    row = torch.from_numpy(np.frombuffer(small.krows[2], dtype=np.uint8).copy()).to(dev)
    for r0 in range(0, T, 8192):
        ok = (text[r0 : r0 + 8192, 2 : W - 1] == row).all(dim=1)
        assert bool(ok.all()), f"line {r0 + int(torch.nonzero(~ok)[0])} does not hold the feature row"
    assert dest.margins_intact() and bool((dest.buf[dest.lead + total : dest.lead + dest.cap] == FILL).all())
    del text, dest, inp
    torch.cuda.empty_cache()


# ---- 5. bad records, late -----------------------------------------------------------------------------------------------------------------
PLAIN_POS = 1


def _with_plain_record(case, s, k):
    """The case with record k of sentence s made a plain known record (id 1, one byte at position 1) -> (case, flat record index, B)."""
    utf8, offsets, tokens, tok_offsets = case
    B = int(offsets[s + 1] - offsets[s])
    r = int(tok_offsets[s]) + k
    assert B >= 2 and r < int(tok_offsets[s + 1])
    tokens = tokens.copy()
    tokens[r] = (1, R.KNOWN, PLAIN_POS, 7, 9, 1)
    return (utf8, offsets, tokens, tok_offsets), r, B


def _case_for_bad_records(d, place):
    for seed in range(100, 140):   # (the first seed whose sentence has two bytes or more)
        rng = np.random.default_rng(seed)
        if place == "far":
            case, s, k = R.many_case(rng, 70001, d.nk, d.nu, long_at=(40000,)), 40000, 150
        else:
            case, s, k = R.make_records(rng, 3, np.array([3, 300, 2]), R.KINDS, d.nk, d.nu), 1, {"token0": 0, "token64": 64, "token200": 200}[place]
        if int(case[1][s + 1] - case[1][s]) >= 2:
            return _with_plain_record(case, s, k)
    raise AssertionError("no seed gave the sentence two bytes")


COLS = {"id": 0, "cls": 1, "position": 2, "byte_len": 5}   # kgpu_token as six 32-bit words


@pytest.mark.parametrize("place", ["token0", "token64", "token200", "far"])
def test_one_bad_record(synth_d, place):
    """One bad record at a time -- id n_morphs + 1, id -1, class 3, position B + 1, byte_len B - position + 1 -- at token 0, 64 or 200 of a
    300-record sentence, or in sentence 40 000 of 70 001 (which only the second trip of the grid-stride loop reaches): kgpu_ctx_sync_lines
    returns KGPU_ERR_INVALID_ARG, the margins stay intact, and with the record put back the same context renders the reference bytes."""
    from kanpyo_amd import _lib

    d = synth_d
    case, r, B = _case_for_bad_records(d, place)
    want, want_off = d.render(case)
    inp = _Input(case)
    _check(d, inp, want, want_off, 3)
    good = inp.tok[r].clone()
    for field, value in [("id", d.nk + 1), ("id", -1), ("cls", 3), ("position", B + 1), ("byte_len", B - PLAIN_POS + 1)]:
        inp.tok[r, COLS[field]] = value
        dest = _Dest(inp.n, len(want) + 32, 3)
        _enqueue(d.ctx, inp, dest)
        rc, _ = _sync(d.ctx)
        assert rc == _lib.KGPU_ERR_INVALID_ARG, (field, value, rc)
        assert "outside the dictionary" in _lib.lib().kgpu_last_error().decode()
        assert dest.margins_intact(), (field, value)
        dest.offsets()
        inp.tok[r] = good
        _check(d, inp, want, want_off, 3)


def test_token_offsets_that_run_backwards(synth_d):
    """tok_offsets[s + 1] < tok_offsets[s] (`bad |= k1 < k0` in k_lines_len)."""
    from kanpyo_amd import _lib

    d = synth_d
    case, _, _ = _case_for_bad_records(d, "token0")
    want, want_off = d.render(case)
    inp = _Input(case)
    assert int(case[3][1]) == 3
    inp.toff[2] = 2   # sentence 1 runs from record 3 to record 2; sentence 2 from record 2 to the end, inside the array
    dest = _Dest(inp.n, len(want) + 4096, 3)
    _enqueue(d.ctx, inp, dest)
    rc, _ = _sync(d.ctx)
    assert rc == _lib.KGPU_ERR_INVALID_ARG and dest.margins_intact()
    inp.toff[2] = int(case[3][2])
    _check(d, inp, want, want_off, 3)


# ---- 6. the protocol around the report words ------------------------------------------------------------------------------------------------
def test_three_renders_without_a_sync_between(synth_d):
    """n = 8, then 70 001, then 8 on one context, each with buffers of its own: an enqueue syncs the render before it (and the scratch of
    sentence lengths grows between the first and the second); kgpu_ctx_sync_lines reports the last."""
    import torch

    from kanpyo_amd import _lib

    from kanpyo_amd.device import DeviceContext

    d = synth_d
    ctx = DeviceContext(d.tok)   # a fresh one: its scratch starts at the size of the first render
    cases = [R.many_case(np.random.default_rng(61), 8, d.nk, d.nu, long_at=(2,)),
             R.many_case(np.random.default_rng(62), 70001, d.nk, d.nu, long_at=(0, 32768, 70000)),
             R.many_case(np.random.default_rng(63), 8, d.nk, d.nu, long_at=(5,))]
    wants = [d.render(c) for c in cases]
    assert len({len(w[0]) for w in wants}) == 3
    inps = [_Input(c) for c in cases]
    dests = [_Dest(i.n, len(w[0]) + 32, mis) for i, w, mis in zip(inps, wants, (13, 6, 1))]
    for i, dst in zip(inps, dests):
        _enqueue(ctx, i, dst)
    assert _sync(ctx) == (_lib.KGPU_OK, len(wants[2][0]))
    assert _sync(ctx) == (_lib.KGPU_OK, 0)   # nothing is pending any more
    torch.cuda.synchronize()
    for dst, (want, want_off) in zip(dests, wants):
        dst.holds(want, want_off)
    ctx.close()


def test_capacity_exact_and_short_by_one(synth_d):
    from kanpyo_amd import _lib

    d = synth_d
    case = R.many_case(np.random.default_rng(64), 300, d.nk, d.nu, long_at=(7, 250))
    want, want_off = d.render(case)
    inp = _Input(case)
    for mis in (0, 11):
        dest = _Dest(inp.n, len(want), mis)
        _enqueue(d.ctx, inp, dest)
        assert _sync(d.ctx) == (_lib.KGPU_OK, len(want))
        dest.holds(want, want_off)
        # short by one: the size reported, nothing written (the offsets are: they do not depend on the capacity)
        dest = _Dest(inp.n, len(want), mis)
        _enqueue(d.ctx, inp, dest, capacity=len(want) - 1)
        assert _sync(d.ctx) == (_lib.KGPU_ERR_CAPACITY, len(want))
        dest.holds(b"", want_off)


def test_null_destination(synth_d):
    from kanpyo_amd import _lib

    d = synth_d
    # sentences without records: nothing to write, no buffer needed
    case = R.make_records(np.random.default_rng(65), 9, 0, R.KINDS, d.nk, d.nu)
    inp = _Input(case)
    dest = _Dest(inp.n, 0, 0)
    _enqueue(d.ctx, inp, dest, capacity=0, text_ptr=0)
    assert _sync(d.ctx) == (_lib.KGPU_OK, 0)
    dest.holds(b"", np.zeros(10, dtype=np.uint64))
    # the same call with records: the size comes back
    case = R.make_records(np.random.default_rng(66), 9, 2, R.KINDS, d.nk, d.nu)
    want, want_off = d.render(case)
    inp = _Input(case)
    dest = _Dest(inp.n, 0, 0)
    _enqueue(d.ctx, inp, dest, capacity=0, text_ptr=0)
    assert len(want) > 0 and _sync(d.ctx) == (_lib.KGPU_ERR_CAPACITY, len(want))
    dest.holds(b"", want_off)
