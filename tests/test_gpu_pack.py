"""The model inputs on the device (include/kanpyo_gpu.h, "model inputs"; kgpu_pack.hip): kgpu_pack_device against kgpu_pack_host byte for byte on the CPU
sweep's shapes (tests/test_pack_cpu.py pins the host form against the plain-Python rule and the `tokenizers` library), the capacity protocol with
canaries, Vocab.encode_pairs_tensor end to end against tests/pack_ref.py applied to the same call's encode_tensor output, and the CLI.  No tolerance:
every array is compared exactly.  Every row array of every call has a canary row behind row_capacity x max_length that must stay as it was."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pack_ref as P
from conftest import ROOT
from pack_cases import ragged, sweep_calls

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
ROWS = ("input_ids", "token_type_ids", "attention_mask", "token_index", "spans")


@pytest.fixture(scope="module")
def ctx():
    """A context of the reference's little test dictionary: the pack never looks at a dictionary, the context gives it a stream and the report."""
    from conftest import fixture_dict_parts
    from kanpyo_amd import Dict, Tokenizer
    from kanpyo_amd.device import DeviceContext

    tok = Tokenizer(Dict.from_parts(**fixture_dict_parts()), device=0)
    c = DeviceContext(tok)
    yield c
    c.close()
    tok.close()


def dev_pack(ctx, opts, ids, off_a, off_b=None, spans=None, tix=None, row_capacity=0, type_ids=True, mask=True, shift=0):
    """kgpu_pack_device + kgpu_ctx_sync_lines -> (return code, rows reported, dict of numpy arrays).  Every row array is row_capacity + 1 rows of SENTINEL:
    the last one is the canary behind the capacity.  shift = 1: the int32 row arrays start one element behind a 16-byte boundary (the dword-store path
    at a max_length that is a multiple of 4)."""
    import ctypes as C

    import torch

    from kanpyo_amd import _lib

    dev = torch.device("cuda", 0)
    ML, n = int(opts.max_length), len(off_a) - 1
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(np.int64 if dt == np.uint64 else dt)).to(dev)   # noqa: E731
    ids32 = np.array(ids, dtype=np.int64).astype(np.int32)
    d_ids = up(np.concatenate([ids32, np.zeros(1, dtype=np.int32)]), np.int32)   # (never empty)
    d_offa = up(off_a, np.uint64)
    d_offb = up(off_b, np.uint64) if off_b is not None else None
    d_sin = torch.from_numpy(np.concatenate([np.array(spans, dtype=np.uint32).reshape(-1, 4), np.zeros((1, 4), dtype=np.uint32)]).view(np.int32)).to(dev) if spans is not None else None
    d_tin = up(np.concatenate([np.array(tix, dtype=np.int32), np.zeros(1, dtype=np.int32)]), np.int32) if tix is not None else None
    words = (row_capacity + 1) * ML
    out = {k: torch.full((words + 4,), SENTINEL, dtype=torch.int32, device=dev) for k in ROWS[:4]}
    out["spans"] = torch.full((words, 4), SENTINEL, dtype=torch.int32, device=dev)
    d_roff = torch.full((n + 2,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n + 1,), 0x77, dtype=torch.uint8, device=dev)
    at = lambda k: out[k].data_ptr() + 4 * shift   # noqa: E731
    torch.cuda.synchronize(dev)
    ctx.pack(opts, n, d_ids.data_ptr(), d_offa.data_ptr(), len(ids), at("input_ids"), row_capacity, d_roff.data_ptr(), d_st.data_ptr(),
             d_ids_b=d_ids.data_ptr() if d_offb is not None else 0, d_off_b=d_offb.data_ptr() if d_offb is not None else 0,
             d_type_ids=at("token_type_ids") if type_ids else 0, d_mask=at("attention_mask") if mask else 0,
             d_spans_in=d_sin.data_ptr() if d_sin is not None else 0, d_tix_in=d_tin.data_ptr() if d_tin is not None else 0,
             d_spans=out["spans"].data_ptr() if d_sin is not None else 0, d_tix=at("token_index") if d_tin is not None else 0)
    got = C.c_uint64(0)
    rc = _lib.lib().kgpu_ctx_sync_lines(ctx._h, C.byref(got))
    res = {k: out[k].cpu().numpy()[shift : shift + words].reshape(row_capacity + 1, ML) for k in ROWS[:4]}
    res["spans"] = out["spans"].cpu().numpy().view(np.uint32).reshape(row_capacity + 1, ML, 4)
    res["row_offsets"] = d_roff.cpu().numpy().view(np.uint64)
    res["status"] = d_st.cpu().numpy()
    for k in ROWS[:4]:   # the words around a shifted array are canaries too
        raw = out[k].cpu().numpy()
        assert (raw[:shift] == SENTINEL).all() and (raw[shift + words:] == SENTINEL).all(), k
    return rc, int(got.value), res


def host_pack(opts, ids, off_a, off_b, spans, tix):
    from kanpyo_amd.pack import pack_host

    return pack_host(opts, np.array(ids, dtype=np.int64).astype(np.int32), np.array(off_a, dtype=np.uint64), None, None if off_b is None else np.array(off_b, dtype=np.uint64),
                     None if spans is None else np.array(spans, dtype=np.uint32).reshape(-1, 4), None if tix is None else np.array(tix, dtype=np.int32))


def assert_device_equals_host(res, R, want, n, written, what):
    """Rows [0, R) of every array in `written` equal the host's, every other row -- the canary row included -- is untouched; row_offsets and status are the
    host's, and nothing lies behind them."""
    assert R == int(want["row_offsets"][-1]), what
    assert res["row_offsets"][: n + 1].tobytes() == want["row_offsets"].tobytes() and res["row_offsets"][n + 1] == 2**64 - 1, what
    assert res["status"][:n].tobytes() == want["status"].tobytes() and res["status"][n] == 0x77, what
    for k in ROWS:
        if k in written:
            w = np.ascontiguousarray(want[k]).view(np.uint32).reshape(res[k][:R].shape) if k == "spans" else want[k]
            assert res[k][:R].tobytes() == np.ascontiguousarray(w).tobytes(), (what, k)
            assert (res[k][R:] == SENTINEL).all(), (what, k, "a row at or behind the total was touched")
        else:
            assert (res[k] == SENTINEL).all(), (what, k, "an array that was not given was touched")


def opts_of(o):
    from kanpyo_amd.pack import pack_opts

    return pack_opts(o["max_length"], o["stride"], o["strategy"], o["windows"], o["cls_id"], o["sep_id"], o["pad_id"], o["trim_front"], o["trim_back"])


# ---- 1. the sweep -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length", [3, 5, 7, 8, 64, 65, 512])
def test_device_equals_host_on_the_sweep(ctx, max_length):
    """3, 5, 7, 65: rows that are not 16-byte aligned, dword stores.  8, 64, 512: 16-byte stores -- and the same shapes again one element off the boundary.
    65: one lane past a wavefront.  Every strategy, windows on and off, the trims, strides 0, 1 and w - 1 (step 1: the most rows a sample can have), samples
    without rows between samples with many; spans and token indices given or not, type ids and mask given or not."""
    from kanpyo_amd import _lib

    rng = random.Random(4000 + max_length)
    calls = no_room = many = 0
    for o, la, lb in sweep_calls(max_length, rng, samples_per_call=None if max_length <= 8 else 14 if max_length <= 65 else 6):
        ids, off_a, off_b, spans, tix = ragged(rng, la, lb)
        opts = opts_of(o)
        variant = calls % 4   # 0: everything; 1: no spans, no token indices; 2: spans only, no type ids; 3: no mask, one element off the boundary
        sp = spans if variant in (0, 2, 3) else None
        tx = tix if variant in (0, 3) else None
        want = host_pack(opts, ids, off_a, off_b, sp, tx)
        R = int(want["row_offsets"][-1])
        rc, got, res = dev_pack(ctx, opts, ids, off_a, off_b, sp, tx, row_capacity=R, type_ids=variant != 2, mask=variant != 3, shift=1 if variant == 3 else 0)
        assert rc == _lib.KGPU_OK, (o, variant)
        written = {"input_ids"} | ({"token_type_ids"} if variant != 2 else set()) | ({"attention_mask"} if variant != 3 else set()) | \
                  ({"spans"} if sp is not None else set()) | ({"token_index"} if tx is not None else set())
        assert_device_equals_host(res, got, want, len(la), written, (o, variant))
        rows = np.diff(want["row_offsets"].astype(np.int64))
        no_room += int((want["status"] == P.NO_ROOM).sum())
        many += int((rows > 2 * (max_length - 3)).sum())
        calls += 1
    assert calls >= 12
    if max_length > 3:
        assert no_room > 0
    if max_length >= 7:
        assert many > 0


@pytest.mark.parametrize("n", [0, 1, 300])
def test_batches_of_0_1_and_300_samples(ctx, n):
    """300 samples over more than one workgroup of the length pass and a grid-stride of the rows: stride = w - 1 beside an empty or one-element question,
    documents of 0 .. 3 room elements, every third sample a question that takes the whole room (zero rows) between documents with dozens of rows."""
    from kanpyo_amd import _lib
    from kanpyo_amd.pack import pack_opts

    rng = random.Random(9 + n)
    # (max_length, stride, strategy, the longest document in rooms); stride 11 at max_length 16 is w - 1 beside a question of one element: step 1
    for max_length, stride, strategy, longest in ((16, 11, "only_second", 20), (64, 59, "only_second", 3), (9, 4, "only_first", 3), (16, 0, "longest_first", 3)):
        room = max_length - 3
        fixed = [room if i % 3 == 1 else rng.randrange(0, 2) for i in range(n)]
        cut = [rng.randrange(0, longest * room) for _ in range(n)]
        la, lb = (cut, fixed) if strategy == "only_first" else (fixed, cut)
        ids, off_a, off_b, spans, tix = ragged(rng, la, lb)
        opts = pack_opts(max_length, stride, strategy, strategy != "longest_first", 101, 102, 0)
        want = host_pack(opts, ids, off_a, off_b, spans, tix)
        R = int(want["row_offsets"][-1])
        rc, got, res = dev_pack(ctx, opts, ids, off_a, off_b, spans, tix, row_capacity=R + 2)   # (more capacity than rows: the rest stays as it was)
        assert rc == _lib.KGPU_OK
        assert_device_equals_host(res, got, want, n, set(ROWS), (n, max_length, strategy))
        if n == 300 and strategy != "longest_first":
            assert (want["status"] == P.NO_ROOM).sum() >= 90 and (np.diff(want["row_offsets"].astype(np.int64)) > 12).any()
        if n == 300 and longest == 20:
            assert R > 2048 * 4, "more rows than the write pass has wavefronts: its grid-stride loop goes round"
        if n == 0:
            assert R == 0 and res["row_offsets"][0] == 0


# ---- 2. capacity, bad offsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length,shift", [(8, 0), (8, 1), (7, 0), (512, 0)])
def test_capacity(ctx, max_length, shift):
    from kanpyo_amd import _lib
    from kanpyo_amd.pack import pack_opts

    rng = random.Random(31)
    room = max_length - 3
    la, lb = [1, 0, room, 2], [3 * room, 1, 5, 2 * room + 1]
    ids, off_a, off_b, spans, tix = ragged(rng, la, lb)
    opts = pack_opts(max_length, max(room - 3, 0), "only_second", True, 1, 2, 0)
    want = host_pack(opts, ids, off_a, off_b, spans, tix)
    R = int(want["row_offsets"][-1])
    assert R >= 6 and want["status"].tolist() == [P.CUT, P.OK, P.NO_ROOM, P.CUT]
    rc, got, res = dev_pack(ctx, opts, ids, off_a, off_b, spans, tix, row_capacity=R, shift=shift)
    assert rc == _lib.KGPU_OK
    assert_device_equals_host(res, got, want, 4, set(ROWS), "row_capacity = R")
    rc, got, res = dev_pack(ctx, opts, ids, off_a, off_b, spans, tix, row_capacity=R - 1, shift=shift)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == R, "one row short: the exact count"
    for k in ROWS:
        assert (res[k] == SENTINEL).all(), (k, "a call that reports KGPU_ERR_CAPACITY wrote a row")
    assert res["row_offsets"][:5].tobytes() == want["row_offsets"].tobytes() and res["status"][:4].tobytes() == want["status"].tobytes(), "always written"
    rc, got, res = dev_pack(ctx, opts, ids, off_a, off_b, spans, tix, row_capacity=0, shift=shift)
    assert rc == _lib.KGPU_ERR_CAPACITY and got == R and all((res[k] == SENTINEL).all() for k in ROWS)


def test_bad_offsets_and_argument_errors(ctx):
    from kanpyo_amd import _lib
    from kanpyo_amd.pack import pack_opts

    ids = list(range(10))
    opts = pack_opts(8, 0, "only_first")
    for off in ([0, 4, 11], [4, 0, 10], [0, 2**63, 10]):
        rc, _, res = dev_pack(ctx, opts, ids, off, row_capacity=8)
        assert rc == _lib.KGPU_ERR_INVALID_ARG, off
        assert (res["input_ids"][8] == SENTINEL).all()
    rc, _, _ = dev_pack(ctx, pack_opts(8, 0, "only_second"), ids, [0, 4, 10], [0, 4, 11], row_capacity=8)
    assert rc == _lib.KGPU_ERR_INVALID_ARG
    rc, got, res = dev_pack(ctx, opts, ids, [0, 4, 10], row_capacity=8)   # the context is usable afterwards
    assert rc == _lib.KGPU_OK and got == 2 and res["input_ids"][0].tolist() == [0, 0, 1, 2, 3, 0, 0, 0]
    for bad in (pack_opts(8, 0, "longest_first", True), pack_opts(8, 0, "only_second"), pack_opts(2, 0, "only_first"), pack_opts(8, 6, "only_first")):
        with pytest.raises(_lib.KgpuError) as e:
            dev_pack(ctx, bad, ids, [0, 4, 10], row_capacity=8)
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------------------------
DIRT = "ｱｲｳｶｷｸﾞﾟＡＢＣｘｙｚ０１２３"


def dirty(sents, seed):
    """Every tenth character replaced by a half-width kana or mark, or a full-width letter or digit: NFKC has something to do."""
    rng = np.random.default_rng(seed)
    out = []
    for s in sents:
        chars = list(s)
        for i in range(int(rng.integers(0, 10)), len(chars), 10):
            chars[i] = DIRT[int(rng.integers(0, len(DIRT)))]
        out.append("".join(chars))
    return out


@pytest.fixture(scope="module")
def pipeline():
    """The synthetic dictionary, a WordPiece Vocab over the characters of a small corpus (every character and its ## form, a few left out: unk_id occurs),
    questions (cfg 2 sentences) and documents (cfg 3, and one of 6144 characters: three windows and more at max_length 512).  Made once, never changed."""
    import unicodedata

    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict, device=0)
    tok.set_features(known, unk)
    questions = dirty(synth.make_corpus(sd, 6, 3, "cfg2"), 3)
    docs = dirty(synth.make_corpus(sd, 5, 4, "cfg3") + ["".join(synth.make_corpus(sd, 3, 4, "cfg5"))], 4)   # (the last: 6144 characters)
    chars = sorted({c for s in questions + docs for c in unicodedata.normalize("NFKC", s)})
    kept = [c for i, c in enumerate(chars) if i % 29 != 5]
    vocab = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"] + [c.encode() for c in kept] + [b"##" + c.encode() for c in kept]
    v = tok.words().vocabulary(vocab, 1, 2, 3, wordpiece=True)
    yield v, questions, docs
    v.close()
    tok.close()


def ref_of_encode(enc, n, pair, **o):
    """pack_ref over what encode_tensor(return_spans=True) returned for first + second: the lists, and per row element the ragged element it came from."""
    ids, off = enc[0].cpu().numpy().tolist(), enc[1].cpu().numpy().tolist()
    spans, tix = enc[3].cpu().numpy().view(np.uint32).tolist(), enc[4].cpu().numpy().tolist()
    off_a, off_b = off[: n + 1], (off[n:] if pair else None)
    ref = P.pack(ids, off_a, ids if pair else None, off_b, spans_in=[tuple(s) for s in spans], tix_in=tix, **o)
    prov = P.pack(ids, off_a, ids if pair else None, off_b, tix_in=list(range(len(ids))), **o)["token_index"]   # the element index rides as a "token index"
    return ref, prov, spans


@pytest.mark.parametrize("pair,max_length,stride,truncation", [(True, 64, 16, "only_second"), (False, 48, 8, "only_second"), (True, 40, 0, "longest_first"),
                                                               (True, 512, 128, "only_second")])
def test_encode_pairs_tensor_end_to_end(pipeline, pair, max_length, stride, truncation):
    import torch

    v, questions, docs = pipeline
    first = (questions + [""]) if pair else docs + ["", questions[0]]
    second = (docs + [docs[0]]) if pair else None
    n = len(first)
    out = v.encode_pairs_tensor(first, second, max_length=max_length, stride=stride, truncation=truncation, pad_id=0, normalize="NFKC", return_spans=True)
    enc = v.encode_tensor(first + (second or []), normalize="NFKC", return_spans=True)
    strategy = {"only_second": P.ONLY_SECOND if pair else P.ONLY_FIRST, "longest_first": P.LONGEST_FIRST}[truncation]
    ref, prov, ragged_spans = ref_of_encode(enc, n, pair, max_length=max_length, stride=stride, strategy=strategy, windows=truncation != "longest_first",
                                            cls_id=2, sep_id=3, pad_id=0, trim_front=1, trim_back=1)
    want = P.as_arrays(ref, max_length)
    R = len(ref["input_ids"])
    assert all(t.is_cuda for t in out.values()) and out["input_ids"].dtype == torch.int32 and tuple(out["spans"].shape) == (R, max_length, 4)
    for k in ("input_ids", "token_type_ids", "attention_mask", "token_index"):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    assert np.array_equal(out["spans"].cpu().numpy().view(np.uint32), want["spans"])
    assert np.array_equal(out["row_offsets"].cpu().numpy().astype(np.uint64), want["row_offsets"]) and np.array_equal(out["status"].cpu().numpy(), want["status"])
    rows = np.diff(want["row_offsets"].astype(np.int64))
    sor = out["sample_of_row"].cpu().numpy()
    assert sor.dtype == np.int64 and np.array_equal(sor, np.repeat(np.arange(n), rows)), "sample_of_row is consistent with row_offsets"
    if truncation != "longest_first":
        assert rows.max() >= 3, "a document long enough for three windows"
    assert (rows == 1).any()
    # every element that is no special: the source text cut by its span is the text cut by the ragged span it came from, in the sentence it came from
    got_spans, types, checked = out["spans"].cpu().numpy().view(np.uint32), want["token_type_ids"], 0
    for r in range(R):
        i = int(sor[r])
        for j in range(max_length):
            e = prov[r][j]
            if e < 0:
                assert got_spans[r, j].tolist() == [0, 0, 0, 0] and want["token_index"][r, j] == -1
                continue
            src = (second[i] if types[r, j] else first[i]).encode()
            p, ln, cs, ce = got_spans[r, j].tolist()
            q, qn, qs, qe = ragged_spans[e]
            assert src[p : p + ln] == src[q : q + qn] and src.decode()[cs:ce] == src.decode()[qs:qe] == src[p : p + ln].decode()
            checked += 1
    assert checked > 200
    plain = v.encode_pairs_tensor(first, second, max_length=max_length, stride=stride, truncation=truncation, normalize="NFKC")
    assert "spans" not in plain and "token_index" not in plain and np.array_equal(plain["input_ids"].cpu().numpy(), want["input_ids"])


def test_a_vocab_without_specials_needs_them_given(pipeline):
    v, questions, docs = pipeline
    bare = v._tokenizer.words().vocabulary(v.words, 1, wordpiece=True)
    try:
        with pytest.raises(ValueError):
            bare.encode_pairs_tensor(questions[:2], docs[:2], max_length=32)
        out = bare.encode_pairs_tensor(questions[:2], docs[:2], max_length=32, stride=4, cls_id=2, sep_id=3)
        want = v.encode_pairs_tensor(questions[:2], docs[:2], max_length=32, stride=4)   # (the trims make the two handles agree)
        assert np.array_equal(out["input_ids"].cpu().numpy(), want["input_ids"].cpu().numpy()) and out["input_ids"].shape[0] > 2
    finally:
        bare.close()


# ---- 4. the CLI ----------------------------------------------------------------------------------------------------------------------------------------
def test_cli_max_length(pipeline, tmp_path):
    from kanpyo_amd import synth
    from kanpyo_amd.dictfile import DictFile, save_dict

    v, questions, docs = pipeline
    sd = synth.build_dict(20000, seed=5)
    known, unk = synth.feature_tables(sd)
    path = tmp_path / "t.dict"
    save_dict(DictFile(sd.dict, known, unk), str(path))
    vfile = tmp_path / "vocab.txt"
    vfile.write_bytes(b"".join(w + b"\n" for w in v.words))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "kanpyo_amd", "encode", "-c", str(path), "--vocab", str(vfile), "--wordpiece", "--unk", "[UNK]", "--bos", "[CLS]", "--eos", "[SEP]",
           "--normalize", "nfkc"]
    pairs = list(zip(questions[:3], docs[-3:]))
    data = "".join(f"{a}\t{b}\n" for a, b in pairs).encode()
    r = subprocess.run(cmd + ["--max-length", "48", "--stride", "8", "--pair"], input=data, capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    out = v.encode_pairs_tensor([a for a, _ in pairs], [b for _, b in pairs], max_length=48, stride=8, normalize="NFKC")
    ids, mask, sor = out["input_ids"].cpu().numpy(), out["attention_mask"].cpu().numpy(), out["sample_of_row"].cpu().numpy()
    expect = "".join("%d\t%s\n" % (sor[k], " ".join(map(str, ids[k][mask[k] == 1].tolist()))) for k in range(ids.shape[0]))
    assert r.stdout.decode() == expect and ids.shape[0] > 6
    single = "".join(d + "\n" for d in docs[:2]).encode()
    r = subprocess.run(cmd + ["--max-length", "32", "--truncation", "longest_first"], input=single, capture_output=True, env=envv, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    out = v.encode_pairs_tensor(docs[:2], None, max_length=32, truncation="longest_first", normalize="NFKC")
    assert r.stdout.decode() == "".join("%d\t%s\n" % (k, " ".join(map(str, out["input_ids"][k].cpu().numpy().tolist()))) for k in range(2))
