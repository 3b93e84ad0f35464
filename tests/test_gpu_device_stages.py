"""The stages of Vocab.encode_tensor / encode_pairs_tensor (normalise, tokenize, encode, pack) and their one more attempt when a first capacity was
too small.  The fixture dictionary, a WordPiece list with [CLS] / [SEP]; DeviceContext's enqueue methods are wrapped and counted.  Whether a stage
fits its first capacity is decided by the references alone (unicodedata, the oracle's records, wordpiece_ref's ids) before anything runs: a stage
that fits is enqueued once, one that does not exactly twice, the second time with the size the first one reported (and 64 for the tokenize).
The tokenize stage's own repeat needs more than bytes / 2 + n + 64 records of a batch, which no text gives on this dictionary (a record has a byte
at least, two for all but ASCII): tests/test_device_calls_cpu.py pins that repeat on the loop itself."""
import numpy as np
import pytest

import align_ref as A
import normalize_ref as N
import wordpiece_ref as WP
from record_cases import LIST, SMALL_KEYS, ref_spec
from record_cases import plain_small_env as small_env  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CAPACITY_AT = {"normalize": (4,), "normalize_aligned": (4, 8), "tokenize": (5,), "encode": (7,), "encode_spans": (7,), "pack": (6,)}   # among the arguments


@pytest.fixture
def calls(monkeypatch):
    """[(method, capacity...)] of every enqueue through DeviceContext, in order."""
    from kanpyo_amd.device import DeviceContext

    log = []
    for name, at in CAPACITY_AT.items():
        def counted(self, *args, _real=getattr(DeviceContext, name), _name=name, _at=at, **kw):
            log.append((_name,) + tuple(args[i] for i in _at))
            return _real(self, *args, **kw)

        monkeypatch.setattr(DeviceContext, name, counted)
    return log


@pytest.fixture(scope="module")
def vocab(small_env):
    v = small_env.words().vocabulary(LIST, 1, 2, 3, wordpiece=True)
    yield v
    v.close()


def reference(env, lines, form=None):
    """-> (bytes, records, edits, (ids, id_offsets)) of the batch by unicodedata, the oracle and wordpiece_ref."""
    raw = [ln.encode() for ln in lines]
    n_edits = 0
    if form is None:
        utf8, offs = np.frombuffer(b"".join(raw), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
    else:
        utf8, offs, status, edits, _ = A.expected_lines(raw, form)
        assert not status.any()
        n_edits = len(edits)
    exp = env.orc.tokenize_batch(utf8, offs, 8)
    want = WP.encode(utf8, offs, exp.tokens, exp.offsets, env.known, env.unk, env.nk, env.nu, ref_spec(), SMALL_KEYS, LIST, 1, 2, 3)
    return len(utf8), len(exp.tokens), n_edits, want


def expected_calls(lines, form, spans, ref):
    """What the stages must enqueue, from the first capacities and the reference's sizes alone."""
    n, total = len(lines), sum(len(ln.encode()) for ln in lines)
    n_bytes, n_records, n_edits, want = ref
    out = []
    if form is not None:
        first, need = (total * 2 + 64, total // 8 + 64), (n_bytes, n_edits)
        if not spans:
            first, need = first[:1], need[:1]
        name = "normalize_aligned" if spans else "normalize"
        out.append((name,) + first)
        if any(k > c for k, c in zip(need, first)):
            out.append((name,) + tuple(max(c, k) for k, c in zip(need, first)))
    cap = n_bytes // 2 + n + 64
    assert n_records <= cap, "no batch of this dictionary outgrows the first token capacity"
    out.append(("tokenize", cap))
    name, cap = "encode_spans" if spans else "encode", n_records + 2 * n
    out.append((name, cap))
    if len(want[0]) > cap:
        out.append((name, len(want[0])))
    return out


def run(vocab, lines, want, **kw):
    got = vocab.encode_tensor(lines, **kw)
    assert len(got) == (5 if kw.get("return_spans") else 3) and not got[2].cpu().numpy().any()
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy().astype(np.uint64), want[1])
    return got


@pytest.mark.parametrize("spans", [False, True])
def test_an_encode_stage_too_small_is_enqueued_twice(small_env, vocab, calls, spans):
    ref = reference(small_env, ["テスト"])
    assert ref[1] == 2 and len(ref[3][0]) == 5, "the token and EOS; three pieces between [CLS] and [SEP]: five ids for a first capacity of four"
    name = "encode_spans" if spans else "encode"
    want = [("tokenize", 9 // 2 + 1 + 64), (name, 4), (name, 5)]
    assert expected_calls(["テスト"], None, spans, ref) == want
    run(vocab, ["テスト"], ref[3], return_spans=spans)
    assert calls == want
    # a sentence that fits: once each.  Padded: the capacity is the caller's n x width, never repeated, and the row is cut
    del calls[:]
    ref = reference(small_env, ["辞書"])
    assert len(ref[3][0]) == 3
    run(vocab, ["辞書"], ref[3], return_spans=spans)
    assert calls == [("tokenize", 6 // 2 + 1 + 64), (name, 4)] == expected_calls(["辞書"], None, spans, ref)
    del calls[:]
    ids = vocab.encode_tensor(["テスト"], width=4, pad_id=0, return_spans=spans)[0]
    assert calls == [("tokenize", 69), (name, 4)] and np.array_equal(ids.cpu().numpy(), WP.padded(*reference(small_env, ["テスト"])[3], 4, 0, 3))


@pytest.mark.parametrize("spans", [False, True])
def test_a_normalise_stage_too_small_is_enqueued_twice(small_env, vocab, calls, spans):
    name = "normalize_aligned" if spans else "normalize"
    # NFC of a short ASCII line stays within its capacity: once
    ref = reference(small_env, ["abc def"], "NFC")
    assert ref[0] == 7
    want = expected_calls(["abc def"], "NFC", spans, ref)
    assert [c[0] for c in want][:2] == [name, "tokenize"] and want[0][1] == 7 * 2 + 64
    run(vocab, ["abc def"], ref[3], normalize="NFC", return_spans=spans)
    assert calls == want
    if not N.versions_agree():
        pytest.skip("Python's unicodedata and the committed tables are of different Unicode versions: no reference for U+FDFA")
    # forty U+FDFA: 120 bytes, a first capacity of 304, 1320 bytes in NFKC
    del calls[:]
    line = "ﷺ" * 40
    ref = reference(small_env, [line], "NFKC")
    assert len(line.encode()) == 120 and ref[0] == 1320 > 304 and ref[2] <= 120 // 8 + 64
    want = expected_calls([line], "NFKC", spans, ref)
    assert want[:3] == [(name, 304) + ((79,) if spans else ()), (name, 1320) + ((79,) if spans else ()), ("tokenize", 1320 // 2 + 1 + 64)]
    run(vocab, [line], ref[3], normalize="NFKC", return_spans=spans)
    assert calls == want


def test_a_pack_stage_that_fits_is_enqueued_once(small_env, vocab, calls):
    ref = reference(small_env, ["テスト"])
    out = vocab.encode_pairs_tensor(["テスト"], max_length=8)
    assert calls == [("tokenize", 69), ("encode", 4), ("encode", 5), ("pack", 1 + 5 // 5 + 8)]
    assert out["input_ids"].cpu().numpy().tolist() == [ref[3][0].tolist() + [0, 0, 0]] and out["row_offsets"].cpu().tolist() == [0, 1]
