"""The five kept-lattice calls as ONE family (kanpyo_amd/csrc/kgpu_lattice_call.h: kgpu_graphviz_batch, kgpu_tokenize_batch_nbest, _marginals, _samples
and _mode share a frame and a context's buffers): interleaved on one handle they give what each gives alone, a call without sentences writes its zeros
and nothing else, and a buffer that overflows in a late chunk is reported with the exact totals.  What each call computes is pinned by its own file
(test_gpu_graphviz.py, test_gpu_nbest.py, test_gpu_prob.py, test_gpu_mode.py); here the calls are compared with themselves.  Every array is filled with
0xA5 before a call and compared WHOLE, so an equal result also says that nothing outside the delivered part was written."""
import ctypes as C

import numpy as np
import pytest

from conftest import fixture_dict_parts, load_golden
from nbest_cases import FIXTURE_INPUTS

pytestmark = pytest.mark.gpu

# 10 sentences: four chunks of at most 3, an invalid and an empty sentence inside chunks, the last chunk one sentence that has output
SENTENCES = FIXTURE_INPUTS[:3] + [b"\xff"] + FIXTURE_INPUTS[3:5] + [""] + ["テストテスト", "あテ", FIXTURE_INPUTS[5]]
HOOKS = ("GRAPHVIZ", "NBEST", "PROB", "MODE")
FILL = 0xA5
ROOMY = (1 << 18, 64)   # capacities nothing here reaches: text bytes or records, paths


def _new_tok():
    from kanpyo_amd import Dict, Tokenizer, _lib
    from kanpyo_amd.dictfile import MorphFeatureTable

    assert _lib.lib().kgpu_device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    g, p = load_golden("fixture_graphviz.json"), fixture_dict_parts()
    tok = Tokenizer(Dict.from_parts(**p))
    tok.set_features(MorphFeatureTable.from_features([g["features"]["known"].get(str(i), ["名詞", f"k{i}", "*"]) for i in range(1, len(p["morphs"]) + 1)]),
                     MorphFeatureTable.from_features([g["features"]["unknown"][str(i)] for i in range(1, len(p["unk_morphs"]) + 1)]))
    return tok


def _buf(n, dtype):
    a = np.empty(max(int(n), 1), dtype=dtype)
    a.view(np.uint8)[:] = FILL
    return a


def _packed(sents):
    from kanpyo_amd.tokenizer import pack_sentences, ptr

    utf8, offs = pack_sentences(sents)
    return ptr(utf8), offs, len(sents), utf8   # (utf8 is kept alive by the caller's tuple)


# One function per call: (tok, packed input, (capacity, path capacity)) -> (rc, {name: array}, totals).  `totals` are (bytes,), (records,) or (records, paths).
def _graphviz(tok, inp, caps):
    from kanpyo_amd import _lib

    u, o, n, _ = inp
    a = dict(text=_buf(caps[0], np.uint8), text_offsets=_buf(n + 1, np.uint64), status=_buf(n, np.uint8))
    got = C.c_uint64(0)
    rc = _lib.lib().kgpu_graphviz_batch(tok.handle, u, o.ctypes.data, n, 48, 0, a["text"].ctypes.data, caps[0], a["text_offsets"].ctypes.data, a["status"].ctypes.data, C.byref(got))
    return rc, a, (got.value,)


def _paths(fn_name, lead):
    def call(tok, inp, caps):
        from kanpyo_amd import _lib
        from kanpyo_amd.tokenizer import TOKEN_DTYPE

        u, o, n, _ = inp
        a = dict(tokens=_buf(caps[0], TOKEN_DTYPE), path_offsets=_buf(n + 1, np.uint64), tok_offsets=_buf(caps[1] + 1, np.uint64), costs=_buf(caps[1], np.int32), status=_buf(n, np.uint8))
        P, T = C.c_uint64(0), C.c_uint64(0)
        rc = getattr(_lib.lib(), fn_name)(tok.handle, u, o.ctypes.data, n, *lead, a["tokens"].ctypes.data, caps[0], a["path_offsets"].ctypes.data, a["tok_offsets"].ctypes.data,
                                          a["costs"].ctypes.data, caps[1], a["status"].ctypes.data, C.byref(P), C.byref(T))
        return rc, a, (T.value, P.value)
    return call


def _marginals(tok, inp, caps):
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    u, o, n, _ = inp
    a = dict(tokens=_buf(caps[0], TOKEN_DTYPE), probs=_buf(caps[0], np.float64), on_best=_buf(caps[0], np.uint8), tok_offsets=_buf(n + 1, np.uint64),
             log_z=_buf(n, np.float64), best_logprob=_buf(n, np.float64), status=_buf(n, np.uint8))
    T = C.c_uint64(0)
    rc = _lib.lib().kgpu_tokenize_batch_marginals(tok.handle, u, o.ctypes.data, n, _lib.KGPU_THETA_DEFAULT, _lib.KGPU_MARGINAL_ALL, 0.0, a["tokens"].ctypes.data, caps[0],
                                                  a["probs"].ctypes.data, a["on_best"].ctypes.data, a["tok_offsets"].ctypes.data, a["log_z"].ctypes.data,
                                                  a["best_logprob"].ctypes.data, a["status"].ctypes.data, C.byref(T))
    return rc, a, (T.value,)


def _mode(tok, inp, caps):
    from kanpyo_amd import _lib
    from kanpyo_amd.mode import mode_opts
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    u, o, n, _ = inp
    a = dict(tokens=_buf(caps[0], TOKEN_DTYPE), tok_offsets=_buf(n + 1, np.uint64), costs=_buf(n, np.int32), status=_buf(n, np.uint8))
    T = C.c_uint64(0)
    opts = mode_opts("search")
    rc = _lib.lib().kgpu_tokenize_batch_mode(tok.handle, u, o.ctypes.data, n, C.byref(opts), a["tokens"].ctypes.data, caps[0], a["tok_offsets"].ctypes.data, a["costs"].ctypes.data,
                                             a["status"].ctypes.data, C.byref(T))
    return rc, a, (T.value,)


def _calls():
    from kanpyo_amd import _lib

    return [("graphviz", _graphviz), ("nbest", _paths("kgpu_tokenize_batch_nbest", (3,))), ("marginals", _marginals),
            ("samples", _paths("kgpu_tokenize_batch_samples", (_lib.KGPU_THETA_DEFAULT, 3, 7))), ("mode", _mode)]


def _chunks_of_three(monkeypatch):
    for h in HOOKS:
        monkeypatch.setenv(f"KGPU_HOST_{h}_CHUNK_SENTS", "3")


def _same(got, want, what):
    rc, arrays, totals = got
    assert rc == want[0] and totals == want[2], (what, rc, totals, want[0], want[2])
    for name, w in want[1].items():
        assert arrays[name].tobytes() == w.tobytes(), (what, name)


@pytest.fixture(scope="module")
def alone():
    """Each call's result when it is the first thing a fresh Tokenizer does, in chunks of three (computed once, left unchanged)."""
    mp = pytest.MonkeyPatch()
    _chunks_of_three(mp)
    try:
        inp = _packed(SENTENCES)
        out = {name: call(_new_tok(), inp, ROOMY) for name, call in _calls()}
    finally:
        mp.undo()
    for name, (rc, arrays, totals) in out.items():
        assert rc == 0 and totals[0] > 0, (name, rc, totals)
        assert arrays["status"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0], name
    return out


def test_interleaved_on_one_handle(alone, monkeypatch):
    """Every call re-lays-out the context's shared buffers (descriptors, per-chunk words, output block) four times; whatever ran before it, its arrays are
    the ones it gives alone."""
    _chunks_of_three(monkeypatch)
    tok, inp, calls = _new_tok(), _packed(SENTENCES), _calls()
    for name, call in calls + calls[::-1]:
        _same(call(tok, inp, ROOMY), alone[name], name)


def test_no_sentences():
    """n = 0: KGPU_OK, offsets[0] = 0, zero totals, and not a byte else."""
    tok = _new_tok()
    inp = (None, np.zeros(1, dtype=np.uint64), 0, None)
    for name, call in _calls():
        rc, arrays, totals = call(tok, inp, (4, 4))
        assert rc == 0 and not any(totals), (name, rc, totals)
        for key, a in arrays.items():
            raw = a.view(np.uint8)
            if key in ("text_offsets", "path_offsets", "tok_offsets"):
                assert int(a[0]) == 0 and (raw[8:] == FILL).all(), (name, key)
            else:
                assert (raw == FILL).all(), (name, key)


def test_overflow_in_a_late_chunk(alone, monkeypatch):
    """A capacity one short of the exact total overflows in the last chunk that has output: KGPU_ERR_CAPACITY, and the need reported is the exact total -- the
    counting went on.  mode's tok_offsets are the exact ones all the same.  The handle's next ordinary call is untouched by it."""
    from kanpyo_amd import _lib

    _chunks_of_three(monkeypatch)
    tok, inp = _new_tok(), _packed(SENTENCES)
    for name, call in _calls():
        exact = alone[name][2]
        short = [(exact[0] - 1, exact[1] if len(exact) > 1 else 0)]
        if len(exact) > 1:
            short.append((exact[0], exact[1] - 1))   # the paths, not the records, are what does not fit
        for caps in short:
            rc, arrays, totals = call(tok, inp, caps)
            assert rc == _lib.KGPU_ERR_CAPACITY and totals == exact, (name, caps, rc, totals, exact)
            if name == "mode":
                assert arrays["tok_offsets"].tobytes() == alone[name][1]["tok_offsets"].tobytes()
        _same(call(tok, inp, ROOMY), alone[name], name)
