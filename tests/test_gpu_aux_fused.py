"""Scan + compaction behind a chain (kanpyo_amd/csrc/kgpu_kernels.hip: launch_scan_compact): the ONE launch without LDS (k_aux_one_launch) against the
two launches (k_scan_counts or, without LDS, k_scan_counts_wave + k_compact / k_compact8), each forced with KGPU_AUX_LAUNCH -- a context reads it when it is
created -- and the chain's own choice, through a device context over the fixture dictionary.  Every arm is compared with the oracle and with the two-launch arm: records, token
offsets, status, the token count.  Which kernels a context launched is asserted (kgpu_debug_aux_form), not assumed from the knob.

Batch sizes: 0, 1, G - 1, G, G + 1 (G = 4 sentences per wavefront up to 4096), the workgroup (256 +- 1), 1024 +- 1, the chain's limit
AUX_ONE_LAUNCH_MAX = 4096 and its neighbours (4097 forced: G = 8).  Sentences: empty, one token, 64, 65 and more than 130 tokens (the copy loop's
strides: 64 lanes a pass, 6 dwords or one 8-byte record a token), invalid UTF-8 (count 0).  Forms: 24-byte records and the compact form.  Capacity:
equal to the total, one below it and half of it -- nothing is written past it, the total and the error are the same.  A second batch on the same
context shows that the control block was left zeroed."""
import numpy as np
import pytest

from conftest import fixture_dict_parts
from kernel_run import libs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = 4
LIMIT = 4096   # kgpu_chain.h: AUX_ONE_LAUNCH_MAX
SIZES = sorted({0, 1, G - 1, G, G + 1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, LIMIT, LIMIT + 1})
ARMS = {"two": "0", "one": "1", "wave": "2", "chain": None}   # KGPU_AUX_LAUNCH: two launches / one / two with the single-wavefront scan / by the chain
WORDS = ["テスト", "辞書", "形態素"]
BAD = b"\xe3\x81"   # a truncated sequence
SENTINEL = 0x5A


def _words(k):
    return "".join(WORDS[i % 3] for i in range(k))


# one period of every batch: the shapes the copy loop and the scan must get right.  Five of its 27 sentences (129 words and more) are too long for the pool
# kernel and go on to the windowed kernel -- more than an eighth: a context's first batch runs behind a chain without small_scan (workgroups of four
# wavefronts), its second behind one with it (of one; the single-wavefront scan when the chain decides).  The test asserts both from the routing counters.
BASE = ["テスト", "", _words(2), "あいうえお", BAD, _words(63), _words(5), "辞書", _words(64), "", _words(65), _words(3), BAD, _words(131),
        "形態素あ", _words(7), "", _words(66), "テスト辞書", _words(200), "あ", _words(62), _words(11), "", _words(129), _words(150), _words(170)]


def _batch(n, shift=0):
    return [BASE[(i + shift) % len(BASE)] for i in range(n)]


@pytest.fixture(scope="module")
def env(libs):
    from kanpyo_amd import Dict, Tokenizer

    _, oracle = libs
    d = Dict.from_parts(**fixture_dict_parts())
    tok, orc = Tokenizer(d), oracle.OracleTokenizer.from_dict(d)
    yield tok, orc, {}
    tok.close()


def _expected(env, n, shift=0):
    """(packed bytes, offsets, expected tokens, expected offsets, expected status) of _batch(n, shift); computed once, left unchanged."""
    from kanpyo_amd import _lib
    from kanpyo_amd.tokenizer import TOKEN_DTYPE, pack_sentences

    tok, orc, cache = env
    if (n, shift) not in cache:
        sents = _batch(n, shift)
        raw = [s if isinstance(s, bytes) else s.encode() for s in sents]
        utf8, offs = pack_sentences(raw)
        valid = [i for i, s in enumerate(sents) if s is not BAD]
        counts = np.zeros(n, dtype=np.uint64)
        status = np.full(n, _lib.KGPU_SENT_INVALID_UTF8, dtype=np.uint8)
        etok = np.empty(0, dtype=TOKEN_DTYPE)
        if valid:
            e = orc.tokenize_batch(*pack_sentences([raw[i] for i in valid]), 2)
            counts[valid] = e.offsets[1:] - e.offsets[:-1]
            status[valid] = 0
            etok = e.tokens
        eoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        if n >= len(BASE):   # the shapes are there: 0, 1, 64, 65 and more than 130 tokens
            c = set(counts.tolist())
            assert {0, 1, 64, 65} <= c and max(c) > 130, sorted(c)
        for a in (utf8, offs, etok, eoff, status):
            a.setflags(write=False)
        cache[(n, shift)] = (utf8, offs, etok, eoff, status)
    return cache[(n, shift)]


class _Ctx:
    """A device context created under one arm of the knob, with the buffers of one batch shape."""

    def __init__(self, tok, arm, monkeypatch):
        from kanpyo_amd.device import PROFILE_OFF, DeviceContext

        if ARMS[arm] is None:
            monkeypatch.delenv("KGPU_AUX_LAUNCH", raising=False)
        else:
            monkeypatch.setenv("KGPU_AUX_LAUNCH", ARMS[arm])
        self.ctx = DeviceContext(tok)
        self.ctx.set_profiling(PROFILE_OFF)

    def run(self, utf8, offs, compact, cap=None, room=None):
        """-> (token count or the KgpuError, records as the buffer holds them [room rows], first or None, token offsets, status)"""
        import torch

        from kanpyo_amd import _lib

        dev = torch.device("cuda", 0)
        n = len(offs) - 1
        room = room if room is not None else int(offs[-1]) + n + 1
        cap = room if cap is None else cap
        assert cap <= room
        d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(1, np.uint8)])).to(dev)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_rec = torch.full((room + 1, 2 if compact else 6), SENTINEL, dtype=torch.int32, device=dev)
        d_first = torch.full((n + 1, 2), SENTINEL, dtype=torch.int32, device=dev)
        d_toff = torch.full((n + 2,), SENTINEL, dtype=torch.int64, device=dev)
        d_st = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device=dev)
        if compact:
            self.ctx.tokenize_compact(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_rec.data_ptr(), cap, d_first.data_ptr(), d_toff.data_ptr(), d_st.data_ptr())
        else:
            self.ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, int(offs[-1]), d_rec.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
        try:
            nt = self.ctx.sync()
        except _lib.KgpuError as e:
            nt = e
        toff, st, first = d_toff.cpu().numpy(), d_st.cpu().numpy(), d_first.cpu().numpy()
        assert toff[n + 1] == SENTINEL and st[n] == SENTINEL and (first[n] == SENTINEL).all(), "written past the per-sentence tables"
        return nt, d_rec.cpu().numpy(), first[:n] if compact else None, toff[:n + 1].astype(np.uint64), st[:n]

    def form(self):
        """what the context's last scan + compaction was, as launch_scan_compact numbers it: 1 the one launch, 3 two launches with the LDS scan, 4 two
        with the single-wavefront scan (kgpu_debug_aux_form, tests only: not in the header)"""
        import ctypes as C

        from kanpyo_amd import _lib

        f = _lib.lib().kgpu_debug_aux_form
        f.argtypes, f.restype = [C.c_void_p], C.c_int
        return int(f(self.ctx._h))

    def close(self):
        self.ctx.close()


def _records(rec, first, toff, nt, compact):
    """the 24-byte records of the first nt rows"""
    from kanpyo_amd.device import expand_tokens
    from kanpyo_amd.tokenizer import TOKEN_DTYPE

    if compact:
        return expand_tokens(rec[:nt].copy(), toff, first)
    return rec[:nt].copy().view(TOKEN_DTYPE).reshape(-1)


def _check(out, exp, compact, what):
    _, _, etok, eoff, est = exp
    nt, rec, first, toff, st = out
    assert nt == len(etok), (what, nt, len(etok))
    assert np.array_equal(toff, eoff), f"{what}: token offsets differ"
    assert np.array_equal(st, est), f"{what}: status differs"
    assert np.array_equal(_records(rec, first, toff, nt, compact), etok), f"{what}: records differ"
    assert (rec[nt:] == SENTINEL).all(), f"{what}: rows behind the records were written"


@pytest.mark.parametrize("compact", [False, True], ids=["rec24", "rec8"])
@pytest.mark.parametrize("n", SIZES)
def test_arms_agree_with_the_oracle_and_each_other(env, n, compact, monkeypatch):
    tok = env[0]
    exp, exp2 = _expected(env, n), _expected(env, n, 7)
    outs = {}
    for arm in ARMS:
        c = _Ctx(tok, arm, monkeypatch)
        try:
            outs[arm] = c.run(exp[0], exp[1], compact)
            # the witness that the arms ran different kernels: the knob was read by this context, and the chain's own choice is the one launch up to
            # the limit (the first batch of a context runs behind a chain without small_scan), two launches above it and for an empty batch
            assert c.form() == {"two": 3, "one": 1, "wave": 4, "chain": 1 if 1 <= n <= LIMIT else 3}[arm], (n, arm, c.form())
            _check(outs[arm], exp, compact, f"n={n} {arm}")
            routed = c.ctx.profile(reset=False)["deferred"][0]
            # a second batch on the same context: the first one left the control block zeroed (its counters are the second's alone)
            second = c.run(exp2[0], exp2[1], compact)
            if arm == "chain" and n:   # an eighth or more of the first batch went on to the windowed kernel: small_scan, the single-wavefront scan
                assert c.form() == (4 if routed * 256 // n >= 32 else 1 if n <= LIMIT else 3), (n, routed, c.form())
                assert n < len(BASE) or routed * 8 >= n, (n, routed)   # ... which a whole period of BASE does
            _check(second, exp2, compact, f"n={n} {arm}, second batch")
            prof = c.ctx.profile()
            assert prof["sentences"] == 2 * n, prof
        finally:
            c.close()
    for arm in ("one", "wave", "chain"):
        for k in (1, 3, 4):   # records, token offsets, status: the whole buffers, sentinels included
            assert np.array_equal(outs[arm][k], outs["two"][k]), (n, arm, k)
        if compact:
            assert np.array_equal(outs[arm][2], outs["two"][2]), (n, arm, "first")
        assert outs[arm][0] == outs["two"][0]


@pytest.mark.parametrize("compact", [False, True], ids=["rec24", "rec8"])
@pytest.mark.parametrize("n", [G + 1, 257, 4096])
def test_capacity(env, n, compact, monkeypatch):
    """out_cap equal to the total, one below it and half of it: a sentence whose records would pass the capacity is not written, nothing is written
    past it, the tables and the total are published all the same, and sync reports KGPU_ERR_CAPACITY with the need -- in both arms alike."""
    from kanpyo_amd import _lib

    tok = env[0]
    exp = _expected(env, n)
    _, _, etok, eoff, est = exp
    total = len(etok)
    assert total >= 8
    for cap in (total, total - 1, total // 2):
        outs = {}
        for arm in ("two", "one"):
            c = _Ctx(tok, arm, monkeypatch)
            try:
                out = c.run(exp[0], exp[1], compact, cap=cap, room=total + 64)
                if cap == total:
                    _check(out, exp, compact, f"n={n} cap={cap} {arm}")
                else:
                    nt, rec, first, toff, st = out
                    assert isinstance(nt, _lib.KgpuError) and nt.code == _lib.KGPU_ERR_CAPACITY and f"need {total}," in str(nt), nt
                    assert np.array_equal(toff, eoff) and np.array_equal(st, est)
                    fits = int(np.searchsorted(eoff, cap, side="right") - 1)   # sentences [0, fits) end at or below the capacity
                    kept = int(eoff[fits])
                    assert (rec[cap:] == SENTINEL).all(), f"n={n} cap={cap} {arm}: written past the capacity"
                    # (an empty sentence behind the capacity writes nothing either way: every row from the first sentence that does not fit is untouched)
                    assert (rec[kept:] == SENTINEL).all(), f"n={n} cap={cap} {arm}: a sentence that does not fit was written"
                    assert np.array_equal(_records(rec, first[:fits] if compact else None, toff[:fits + 1], kept, compact), etok[:kept])
                # the context is usable behind the error
                _check(c.run(exp[0], exp[1], compact), exp, compact, f"n={n} behind cap={cap} {arm}")
                outs[arm] = out
            finally:
                c.close()
        for k in (1, 3, 4):
            assert np.array_equal(outs["one"][k], outs["two"][k]), (n, cap, k)
        if compact:
            assert np.array_equal(outs["one"][2], outs["two"][2])
