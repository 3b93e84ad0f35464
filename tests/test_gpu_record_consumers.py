"""The four consumers of a batch's 24-byte records -- the `kanpyo tokenize` lines, the wakati lines, the vocabulary ids and the word counts -- share one
walk over the sentences and one record check (kanpyo_amd/csrc/kgpu_records_dev.h).  Here ONE crafted batch goes through all four on ONE context: each
must give its own reference's result (tests/lines_ref.py, words_ref.py, encode_ref.py, count_ref.py -- never the library's), the four must agree with
each other on how many words a sentence has, and a record that breaks one of the five rules must be refused by all four.  No tolerance anywhere."""

import numpy as np
import pytest

import encode_ref as E
import lines_ref as R
import words_ref as W
from record_cases import SENTINEL, SMALL_KEYS, _Dest, _enqueue, _Input, _sync, crafted_ids, crafted_want, dev_count, dev_encode, holds, ref_spec, small_env  # noqa: F401  (small_env: the fixture)

pytestmark = pytest.mark.gpu

RECORDS = (0, 1, 63, 64, 65, 128, 129)   # per sentence, cycled: nothing, one, and one less / exactly / one more than one and two windows of 64
N_SENT = 70
BAD_SENTENCE, BAD_RECORD = 64, 100       # ... its second window
SPECS = ({}, {"drop": ("未知",)}, {"keep": ("未知",), "separator": "|"})
MIS = (1, 15)
U, K, D = R.UNKNOWN, R.KNOWN, R.DUMMY


def make_case(nk, nu):
    """70 sentences of 24..40 bytes in '"'..'{': no space, no '|', no newline (a separator in a wakati line is then a separator), sentence s with
    RECORDS[(s + 5) % 7] records -- sentence 64 has 129.  Record k of sentence s is, by (k + s) % 6: a known id 1 or 2, an unknown with an id, a known
    without a row (id 0), the dummy class with noise in every field, an unknown without a row, and known id 3 (the 10 200-byte row) once per long
    sentence.  Every surface has a byte at least, so only a sentence where nothing is kept renders to a lone newline."""
    sents, per = [], []
    for s in range(N_SENT):
        B = 24 + s % 17
        sents.append(bytes((7 * i + 3 * s) % 90 + 34 for i in range(B)))
        recs = []
        for k in range(RECORDS[(s + 5) % len(RECORDS)]):
            pos, bl = (5 * k + s) % (B - 3), 1 + k % 3
            kind = (k + s) % 6
            if kind == 0:
                recs.append((1 + k % 2, K, pos, bl))
            elif kind == 1:
                recs.append((1 + k % nu, U, pos, bl))
            elif kind == 2:
                recs.append((0, K, pos, bl))
            elif kind == 3:
                recs.append(((-7, 0, nk + 9)[k % 3], D, 0xFFFFFFF0 + k % 7, 0x80000000 + k))
            elif kind == 4:
                recs.append((0, U, pos, bl))
            else:
                recs.append((3 if k == 5 else nk - 1, K, B - bl, bl))
        per.append(recs)
    case = R.pack(sents, per)
    counts = np.diff(case[3].astype(np.int64))
    assert set(counts.tolist()) == set(RECORDS) and counts[BAD_SENTENCE] == 129
    assert {int(c) for c in case[2]["cls"]} == {D, K, U} and (case[2]["id"] == 0).any() and (case[2]["id"] < 0).any()
    return case


class _Run:
    """The four consumers on one context that never tokenizes."""

    def __init__(self, env):
        from kanpyo_amd.device import DeviceContext

        self.env = env
        self.ctx = DeviceContext(env.tok)
        self.krows, self.urows = R.rows_of(env.known, env.nk), R.rows_of(env.unk, env.nu)

    def lines(self, inp, cap, mis):
        dest = _Dest(inp.n, cap, mis)
        _enqueue(self.ctx, inp, dest)
        return _sync(self.ctx), dest

    def words(self, inp, kw, cap, mis):
        import torch

        dest = _Dest(inp.n, cap, mis)
        torch.cuda.synchronize()
        self.ctx.format_words(self.env.words(**kw), inp.utf8.data_ptr(), inp.off.data_ptr(), inp.n, inp.tok.data_ptr(), inp.toff.data_ptr(), dest.text_ptr, cap, dest.offs_ptr)
        return _sync(self.ctx), dest

    def vocab_words(self, case, kw):
        env = self.env
        words = [w for s in E.sentence_words(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw), SMALL_KEYS) for w in s]
        return [b"<pad>", b"<unk>"] + sorted(set(words))[::2]


@pytest.fixture(scope="module")
def run(small_env):
    r = _Run(small_env)
    yield r
    r.ctx.close()


@pytest.fixture(scope="module")
def case(small_env):
    return make_case(small_env.nk, small_env.nu)


def _words_in(text, off, sep):
    """Words per sentence of a wakati text whose words hold no separator and are never empty: a lone newline is no word."""
    out = []
    for s in range(len(off) - 1):
        line = text[int(off[s]) : int(off[s + 1])]
        assert line.endswith(b"\n") and line.count(b"\n") == 1
        out.append(0 if line == b"\n" else line.count(sep) + 1)
    return np.array(out, dtype=np.int64)


def test_each_consumer_matches_its_reference_and_they_agree(run, case):
    env = run.env
    inp = _Input(case)
    want_lines = R.render(*case, run.krows, run.urows)
    for mis in MIS:
        (rc, nb), dest = run.lines(inp, len(want_lines[0]) + 32, mis)
        assert (rc, nb) == (0, len(want_lines[0])), (mis, rc, nb)
        dest.holds(*want_lines)
    for kw in SPECS:
        sep = kw.get("separator", " ").encode()
        want = W.render(*case, env.known, env.unk, env.nk, env.nu, ref_spec(**kw))
        for mis in MIS:
            (rc, nb), dest = run.words(inp, kw, len(want[0]) + 32, mis)
            assert (rc, nb) == (0, len(want[0])), (kw, mis, rc, nb)
            dest.holds(*want)
        got = dest.buf.cpu().numpy()[dest.lead : dest.lead + nb].tobytes()
        n_words = _words_in(got, dest.offsets(), sep)
        # the ids, ragged, without bos / eos
        vocab = run.vocab_words(case, kw)
        want_ids = crafted_ids(env, case, kw, vocab, 1)
        v = env.words(**kw).vocabulary(vocab, 1)
        rc, n_ids, buf, ioff = dev_encode(run.ctx, v, case, room=len(want_ids[0]) + 32)
        v.close()
        assert (rc, n_ids) == (0, len(want_ids[0])), (kw, rc, n_ids)
        assert np.array_equal(ioff, want_ids[1]) and np.array_equal(buf[:n_ids], want_ids[0]) and (buf[n_ids:] == SENTINEL).all()
        assert 1 in want_ids[0] and (want_ids[0] > 1).any(), "the list must hold some of the words and miss some"
        # the counts
        want_counts = crafted_want(env, case, kw)
        k = env.words(**kw).counter(table_slots=1 << 12, key_bytes=1 << 18)
        rc, n_counted = dev_count(run.ctx, k, case)
        assert rc == 0
        holds(k, want_counts)
        k.close()
        # ... and across the consumers
        assert np.array_equal(n_words, np.diff(ioff.astype(np.int64))), kw
        assert int(n_words.sum()) == n_counted == sum(want_counts.values()), kw
        assert 0 < n_counted < len(case[2]), "some records are words and some are not"


@pytest.mark.parametrize("what", ["class", "position", "byte_len", "id_above", "id_negative"])
def test_one_bad_record_is_refused_by_all_four(run, case, what):
    from kanpyo_amd import _lib

    env = run.env
    utf8, offsets, tokens, tok_offsets = case
    B = int(offsets[BAD_SENTENCE + 1] - offsets[BAD_SENTENCE])
    r = int(tok_offsets[BAD_SENTENCE]) + BAD_RECORD
    assert 64 <= BAD_RECORD < 128 <= int(tok_offsets[BAD_SENTENCE + 1] - tok_offsets[BAD_SENTENCE])
    bad = tokens.copy()
    bad[r] = {"class": (1, 3, 0, 0, 0, 0), "position": (1, K, B + 1, 0, 0, 0), "byte_len": (1, U, 5, 0, 0, B - 4),
              "id_above": (env.nu + 1, U, 0, 0, 0, 0), "id_negative": (-1, K, 0, 0, 0, 0)}[what]
    bad_case = (utf8, offsets, bad, tok_offsets)
    with pytest.raises(ValueError):
        R.render(*bad_case, run.krows, run.urows)
    with pytest.raises(ValueError):
        W.render(*bad_case, env.known, env.unk, env.nk, env.nu, ref_spec())
    inp = _Input(bad_case)
    cap = len(R.render(*case, run.krows, run.urows)[0]) + 64
    (rc, _), dest = run.lines(inp, cap, 1)
    assert rc == _lib.KGPU_ERR_INVALID_ARG and dest.margins_intact(), what
    (rc, _), dest = run.words(inp, {}, cap, 15)
    assert rc == _lib.KGPU_ERR_INVALID_ARG and dest.margins_intact(), what
    v = env.words().vocabulary([b"<pad>", b"<unk>"], 1)
    rc = dev_encode(run.ctx, v, bad_case, room=len(tokens) + 32)[0]
    v.close()
    assert rc == _lib.KGPU_ERR_INVALID_ARG, what
    k = env.words().counter(table_slots=1 << 12, key_bytes=1 << 18)   # a fresh handle per case
    rc = dev_count(run.ctx, k, bad_case)[0]
    k.close()
    assert rc == _lib.KGPU_ERR_INVALID_ARG, what
    # the same context serves the good batch afterwards
    want = R.render(*case, run.krows, run.urows)
    (rc, nb), dest = run.lines(_Input(case), len(want[0]) + 32, 15)
    assert (rc, nb) == (0, len(want[0]))
    dest.holds(*want)
