"""kgpu_format_lines_device's own checks: a record the tokenizer could not have written (class, morph id or surface out of range) makes
kgpu_ctx_sync_lines return KGPU_ERR_INVALID_ARG -- the range checks that also keep the render from reading outside the feature pool and
the sentence -- and a context whose tokenize batch is not synced yet is refused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    from kanpyo_amd import Tokenizer, synth

    sd = synth.build_dict(20000, seed=11)
    known, unk = synth.feature_tables(sd)
    tok = Tokenizer(sd.dict)
    tok.set_features(known, unk)
    return sd, tok


def _device_batch(tok, sents):
    import torch

    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    utf8, offs = pack_sentences(sents)
    dev = torch.device("cuda", 0)
    n, cap = len(sents), int(offs[-1]) + len(sents)
    b = dict(utf8=torch.from_numpy(utf8.copy()).to(dev), off=torch.from_numpy(offs.astype(np.int64)).to(dev),
             tok=torch.empty((cap, 6), dtype=torch.int32, device=dev), toff=torch.empty(n + 1, dtype=torch.int64, device=dev),
             st=torch.empty(n, dtype=torch.uint8, device=dev), text=torch.zeros(1 << 20, dtype=torch.uint8, device=dev),
             text_off=torch.empty(n + 1, dtype=torch.int64, device=dev), n=n, total=int(offs[-1]), cap=cap)
    ctx = DeviceContext(tok)
    return ctx, b


def _tokenize(ctx, b):
    ctx.tokenize(b["utf8"].data_ptr(), b["off"].data_ptr(), b["n"], b["total"], b["tok"].data_ptr(), b["cap"], b["toff"].data_ptr(), b["st"].data_ptr())


def _render(ctx, b):
    ctx.format_lines(b["utf8"].data_ptr(), b["off"].data_ptr(), b["n"], b["tok"].data_ptr(), b["toff"].data_ptr(), b["text"].data_ptr(),
                     b["text"].numel(), b["text_off"].data_ptr())
    return ctx.sync_lines()


@pytest.mark.parametrize("field,value", [("id", "n_morphs + 1"), ("id", "-5"), ("cls", "7"), ("position", "B + 1"), ("byte_len", "B + 2")])
def test_a_record_out_of_range_is_reported(small, field, value):
    from kanpyo_amd import _lib

    sd, tok = small
    ctx, b = _device_batch(tok, ["すもももももももものうち", "テスト"])
    _tokenize(ctx, b)
    nt = ctx.sync()
    good = _render(ctx, b)
    want = b["text"][:good].cpu().numpy().tobytes()
    assert good > 0 and want.endswith(b"EOS\t\n")
    # a known word's record of the first sentence (its id in 1..n_morphs)
    rec = b["tok"][:nt].cpu().numpy()
    first_len = int(b["toff"][1])
    r = next(i for i in range(first_len) if rec[i][1] == 1)
    B = len("すもももももももものうち".encode())
    col = {"id": 0, "cls": 1, "position": 2, "byte_len": 5}[field]
    v = eval(value, {"n_morphs": tok.info()["n_morphs"], "B": B})
    b["tok"][r, col] = v
    with pytest.raises(_lib.KgpuError) as e:
        _render(ctx, b)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "outside the dictionary" in str(e.value)
    # the records put back: the same bytes as before
    b["tok"][r, col] = int(rec[r][col])
    assert _render(ctx, b) == good and b["text"][:good].cpu().numpy().tobytes() == want
    ctx.close()


def test_an_unsynced_batch_is_refused(small):
    from kanpyo_amd import _lib

    sd, tok = small
    ctx, b = _device_batch(tok, synth_sentences(sd))
    _tokenize(ctx, b)
    with pytest.raises(_lib.KgpuError) as e:
        _render(ctx, b)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG and "not synced" in str(e.value)
    ctx.sync()
    assert _render(ctx, b) > 0
    ctx.close()


def synth_sentences(sd):
    from kanpyo_amd import synth

    return synth.make_corpus(sd, 64, 3, "cfg2")
