"""The text from ids on the device (include/kanpyo_gpu.h, "text from ids"; kgpu_decode.hip): rule 5 -- kgpu_decode_device gives what kgpu_decode_host
gives, text, offsets and status, byte for byte -- on crafted sequences at the window edges, the unit edges and every alignment of the destination; the
capacity protocol; the refusals; the round trip through encode_tensor; the host call, two threads at once; and what a first decode leaves alone."""
import random
import threading

import numpy as np
import pytest

import decode_ref as R
from kanpyo_amd import _lib
from kanpyo_amd.decode import decode_host, decode_opts, lines
from record_cases import FILL, LIST, _Dest, _Env, _sync, small_ctx  # noqa: F401
from record_cases import plain_small_env as small_env  # noqa: F401  (small_ctx, small_env: the fixtures; every EOS of this small_env is reachable)

pytestmark = pytest.mark.gpu

PREFIX = b"##"
# the empty word, the prefix itself, words of 1, 15, 16, 17, 64, 65 and 3072 bytes, continuation words, a doubled prefix
CRAFT = [b"", b"##", b"a", b"##b", b"c" * 15, b"d" * 16, b"##" + b"e" * 15, b"f" * 64, b"g" * 65, bytes(range(1, 256)) * 12 + b"h" * 12, b"####y", b"\xff\xfe", b"##" + b"z" * 62]
EMPTY, PRE, A, CONT_B, C15, D16, CONT_E17, F64, G65, H3072, HASH_Y, NOT_UTF8, CONT_Z64 = range(len(CRAFT))
SEPS = (b"", b" ", b"\xe3\x80\x80", b"<--sep->")
assert [len(CRAFT[k]) for k in (EMPTY, A, C15, D16, CONT_E17, F64, G65, H3072)] == [0, 1, 15, 16, 17, 64, 65, 3072]


@pytest.fixture(scope="module")
def craft(small_env):
    v = small_env.words().vocabulary(CRAFT, 2, wordpiece=True)
    yield v
    v.close()


def dev_decode(ctx, v, ids, offsets=None, width=0, opts=None, mis=0, capacity=None, room=None, ids_shift=0):
    """kgpu_decode_device + kgpu_ctx_sync_lines on ids in device memory -> (return code, bytes reported, the destination, status uint8 [n + 8]).  The ids start
    ids_shift int32s behind a 16-byte boundary; the destination starts `mis` bytes behind one (record_cases._Dest: 0xAB all over, canaries around the
    offsets); the status bytes are n of them in front of 8 bytes of 0xAB."""
    import torch

    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    n = len(offsets) - 1 if offsets is not None else ids.size // width
    raw = np.zeros(ids.size + ids_shift + 1, dtype=np.int32)
    raw[ids_shift : ids_shift + ids.size] = ids
    d_ids = torch.from_numpy(raw).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(dev) if offsets is not None else None
    dest = _Dest(n, room if room is not None else (capacity or 0), mis)
    d_st = torch.full((n + 8,), FILL, dtype=torch.uint8, device=dev)
    assert d_ids.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.decode(v, d_ids.data_ptr() + 4 * ids_shift, d_off.data_ptr() if d_off is not None else 0, n, dest.text_ptr, dest.cap if capacity is None else capacity,
               dest.offs_ptr, d_st.data_ptr(), width=width, opts=opts)
    rc, got = _sync(ctx)
    return rc, got, dest, d_st.cpu().numpy()


def check_rule_5(ctx, v, seqs=None, sep=b" ", skip=(), mis=0, ids_shift=0, padded=None, prefix=PREFIX):
    """One device call against kgpu_decode_host on the same input, at the exact capacity: text, offsets, status, and not a byte elsewhere.  seqs: ragged id
    lists (the ids array starts with two ids nobody owns); padded: (rows, width).  -> the lines."""
    if padded is None:
        offsets = np.cumsum([2] + [len(s) for s in seqs]).astype(np.uint64)
        ids = np.array([A, A] + [i for s in seqs for i in s], dtype=np.int64).astype(np.int32)
        width = 0
    else:
        ids, width = np.array(padded[0], dtype=np.int64).astype(np.int32), padded[1]
        offsets = None
    text, toff, status = decode_host(v.words, ids, offsets, width, prefix, sep, skip)
    rc, got, dest, st = dev_decode(ctx, v, ids, offsets, width, decode_opts(sep, skip), mis=mis, capacity=text.size, ids_shift=ids_shift)
    assert (rc, got) == (0, text.size)
    dest.holds(text.tobytes(), toff)
    assert st[: status.size].tolist() == status.tolist() and (st[status.size :] == FILL).all()
    return lines(text, toff)


# ---- 1. rule 5 on crafted sequences ---------------------------------------------------------------------------------------------------------------------
def window_cases(rng):
    anyid = lambda: rng.choice((EMPTY, PRE, A, CONT_B, C15, D16, CONT_E17, HASH_Y, NOT_UTF8, A, CONT_B))   # noqa: E731
    seqs = [[anyid() for _ in range(n)] for n in (0, 1, 63, 64, 65, 128, 129)]                           # window edges
    seqs.append([-7] * 64 + [CONT_B, A])             # 64 skipped ids: kept element 0 lies in the second window and keeps its prefix
    seqs.append([A] * 64 + [CONT_B, A])              # a continuation piece as element 64: it joins across the window edge
    seqs.append([A] * 64 + [PRE] * 64 + [A])         # a whole window of zero-byte contributors between two words
    seqs.append([EMPTY] + [PRE] * 70 + [CONT_B])     # nothing but zero-byte pieces in front of a continuation: it is NOT element 0
    seqs.append([H3072, G65, F64, D16, C15, CONT_E17, A, EMPTY, CONT_Z64, H3072, CONT_B])   # 16-byte units shared between pieces, windows and sequences
    seqs.append([-7] * 130)                          # every id skipped
    seqs.append([-1, len(CRAFT), 2**31 - 1, -2**31] * 20)   # every id out of range
    seqs.append([A, -1, CONT_B])                     # a bad id between two kept ones gives nothing
    return seqs


@pytest.mark.parametrize("sep", SEPS, ids=["sep0", "sep1", "sep3", "sep8"])
def test_device_equals_host_on_crafted_sequences(small_ctx, craft, sep):
    seqs = window_cases(random.Random(len(sep)))
    got = check_rule_5(small_ctx, craft, seqs, sep, skip=[-7])
    want, want_status = R.decode(CRAFT, seqs, PREFIX, sep, [-7])   # (and the host is what the plain-Python rule says)
    assert got == want and want_status[-3:] == [0, 1, 1]
    assert got[7] == b"##b" + sep + b"a" and got[8] == sep.join([b"a"] * 64) + b"b" + sep + b"a" and got[9] == sep.join([b"a"] * 65) and got[10] == b"b"
    assert got[12] == got[13] == b"" and got[14] == b"ab"


@pytest.mark.parametrize("n", [0, 1, 5, 4 * 64 + 1])
def test_batch_sizes(small_ctx, craft, n):
    rng = random.Random(n)
    seqs = [[rng.randrange(len(CRAFT) - 1) if rng.random() < 0.9 else -1 for _ in range(rng.choice((0, 1, 3, 70)))] for _ in range(n)]
    assert len(check_rule_5(small_ctx, craft, seqs, b" ", mis=n % 16)) == n


@pytest.mark.parametrize("width", [1, 64, 65])
def test_padded_rows(small_ctx, craft, width):
    rng = random.Random(width)
    pad = 99
    rows = []
    for fill in (0, 1, width // 2, width):   # a row of pads alone, ..., a full row
        rows.append([rng.choice((A, CONT_B, C15, EMPTY, CONT_E17)) for _ in range(fill)] + [pad] * (width - fill))
    rows.append([pad] * (width - 1) + [CONT_B])   # pads in front: the continuation piece is kept element 0
    flat = [i for r in rows for i in r]
    got = check_rule_5(small_ctx, craft, padded=(flat, width), skip=[pad])
    assert got[0] == b"" and got[-1] == b"##b" and got == R.decode(CRAFT, rows, PREFIX, b" ", [pad])[0]


@pytest.mark.parametrize("mis", range(16))
def test_every_alignment_of_the_destination_and_of_the_ids(small_ctx, craft, mis):
    seqs = [[A], [C15, CONT_B], [], [D16], [CONT_E17, F64, A], [G65, CONT_Z64], [A, A, A]]
    check_rule_5(small_ctx, craft, seqs, b" ", mis=mis, ids_shift=mis % 4)   # (ids_shift 1..3: 4-byte aligned ids that are not 16-byte aligned)


def test_a_plain_handle_has_no_continuation_words(small_ctx, small_env):
    v = small_env.words().vocabulary(CRAFT, 2)
    got = check_rule_5(small_ctx, v, [[A, CONT_B, PRE, EMPTY, A]], b" ", prefix=b"")
    assert got == [b"a ##b ##  a"]
    v.close()


def test_second_trips_of_the_grid_stride_loop(small_ctx, small_env):
    """More sequences than launch_render's capped grid has wavefronts: every wavefront decodes a second sequence, in LDS rows its first one has used.  The
    sequences are the WordPiece ids (by the reference) of test_gpu_wordpiece_adversarial.py's second-trip batch: 0 to 3 short records each, three long
    ones at sequences 0, 32 768 and the last; ragged, and padded at width 65; the destination 3 bytes behind a 16-byte boundary."""
    import encode_ref as E
    import wordpiece_cases as WC
    import wordpiece_ref as WP
    from record_cases import SMALL_KEYS, ref_spec

    n, vocab = WC.SECOND_TRIP_N, WC.second_trip_list()
    assert n > WC.GRID_BLOCKS * WC.render_wpb()
    recs = WC.second_trip_records(small_env.nk, small_env.nu)
    ids, off = WP.encode(*recs, small_env.known, small_env.unk, small_env.nk, small_env.nu, ref_spec(), SMALL_KEYS, vocab, WC.UNK)
    seqs = R.sequences_of(ids, off)
    L = np.diff(off.astype(np.int64))
    assert len(seqs) == n and all(L[s] > 128 for s in WC.LONG_AT) and int((L[WC.GRID_BLOCKS * WC.render_wpb():] > 0).sum()) > 100 and int((L == 0).sum()) > 1000
    v = small_env.words().vocabulary(vocab, WC.UNK, wordpiece=True)
    want, status = R.decode(vocab, seqs, PREFIX, b" ", [])
    assert not any(status) and len(want[0]) > 200 and len(want[32768]) > 200 and len(want[n - 1]) > 200
    assert check_rule_5(small_ctx, v, seqs, b" ", mis=3) == want
    pad = len(vocab)
    rows = E.padded(ids, off, 65, pad)
    assert rows.shape == (n, 65) and int((L > 65).sum()) == 3 and int((rows[:, -1] != pad).sum()) == 3, "the three long sequences fill their rows, cut"
    cut, status = R.decode(vocab, rows.tolist(), PREFIX, b" ", [pad])
    assert not any(status) and cut[1:32768] == want[1:32768] and cut[0] != want[0]
    assert check_rule_5(small_ctx, v, padded=(rows.reshape(-1), 65), skip=[pad], mis=3) == cut
    v.close()


# ---- 2. capacity, refusals --------------------------------------------------------------------------------------------------------------------------------
def test_capacity_protocol(small_ctx, craft):
    seqs = [[A, CONT_B], [], [H3072, A], [-1]]
    offsets = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    ids = np.array([i for s in seqs for i in s], dtype=np.int32)
    text, toff, status = decode_host(CRAFT, ids, offsets, prefix=PREFIX)
    need = text.size
    assert need == 2 + 3072 + 2
    rc, got, dest, st = dev_decode(small_ctx, craft, ids, offsets, capacity=need, mis=3)   # an exact fit
    assert (rc, got) == (0, need)
    dest.holds(text.tobytes(), toff)
    rc, got, dest, st = dev_decode(small_ctx, craft, ids, offsets, capacity=need - 1, room=need + 64, mis=3)   # one byte less: the size, and no store
    assert (rc, got) == (_lib.KGPU_ERR_CAPACITY, need)
    dest.holds(b"", toff)                                            # the offsets and the status are written all the same (rule 4)
    assert st[:4].tolist() == status.tolist() == [0, 0, 0, 1]
    rc, got, dest, st = dev_decode(small_ctx, craft, ids, offsets, capacity=0, room=16)
    assert (rc, got) == (_lib.KGPU_ERR_CAPACITY, need) and dest.margins_intact()


def test_refusals(small_ctx, small_env, craft):
    import torch

    from kanpyo_amd.device import DeviceContext

    ids, offsets = np.array([A, CONT_B], dtype=np.int32), np.array([0, 2], dtype=np.uint64)
    other = _Env(small_env.dict, small_env.known, small_env.unk)      # a context of another dictionary
    ctx = DeviceContext(other.tok)
    with pytest.raises(_lib.KgpuError) as e:
        dev_decode(ctx, craft, ids, offsets, capacity=16)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    ctx.close()
    for kw in (dict(offsets=offsets, width=2), dict(offsets=None, width=0)):   # both, and neither, of offsets and width
        with pytest.raises(_lib.KgpuError) as e:
            small_ctx.decode(craft, 16, 16 if kw["offsets"] is not None else 0, 1, 16, 16, 16, 16, width=kw["width"])
        assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    with pytest.raises(_lib.KgpuError) as e:
        small_ctx.decode(craft, 18, 16, 1, 16, 16, 16, 16)           # ids that are not 4-byte aligned
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    # one render-kind call is pending per context, as for the other consumers: behind a tokenize batch that is not synced the enqueue is refused;
    # behind a pending decode it waits that one out, and the second's result is the one the sync reports
    dev = torch.device("cuda", 0)
    utf8 = torch.from_numpy(np.frombuffer("テスト".encode() + bytes(16), dtype=np.uint8).copy()).to(dev)
    off = torch.tensor([0, 9], dtype=torch.int64, device=dev)
    tok, toff, st = torch.empty((16, 6), dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    small_ctx.tokenize(utf8.data_ptr(), off.data_ptr(), 1, 9, tok.data_ptr(), 16, toff.data_ptr(), st.data_ptr())
    with pytest.raises(_lib.KgpuError) as e:
        dev_decode(small_ctx, craft, ids, offsets, capacity=16)
    assert e.value.code == _lib.KGPU_ERR_INVALID_ARG
    assert small_ctx.sync() >= 1
    d_ids = torch.from_numpy(np.array([A, CONT_B, C15, 0], dtype=np.int32)).to(dev)
    d_off = torch.tensor([0, 2, 3], dtype=torch.int64, device=dev)
    d_text, d_toff, d_st = torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    small_ctx.decode(craft, d_ids.data_ptr(), d_off.data_ptr(), 1, d_text.data_ptr(), 64, d_toff.data_ptr(), d_st.data_ptr())
    small_ctx.decode(craft, d_ids.data_ptr(), d_off.data_ptr(), 2, d_text.data_ptr(), 64, d_toff.data_ptr(), d_st.data_ptr())
    assert small_ctx.sync_lines() == 17 and d_text.cpu().numpy()[:17].tobytes() == b"ab" + b"c" * 15 and small_ctx.sync_lines() == 0


# ---- 3. the round trip through code that exists ----------------------------------------------------------------------------------------------------------
SENTS = ["テスト辞書", "", "形態素テスト", "辞書形態素辞書"]


def tensor_lines(text, toff):
    return lines(text.cpu().numpy(), toff.cpu().numpy())


def test_round_trip_on_a_plain_list_is_the_wakati_render(small_env):
    w = small_env.words()
    rendered = w.render(SENTS)
    listed = sorted({x for r in rendered for x in r.split(" ") if x})
    v = w.vocabulary(["<unk>"] + listed, 0)
    ids, off, st = v.encode_tensor(SENTS)
    text, toff, status = v.decode_tensor(ids, off)
    assert tensor_lines(text, toff) == [r.encode() for r in rendered] and status.cpu().tolist() == [0] * len(SENTS)
    assert (str(text.dtype), str(toff.dtype), str(status.dtype)) == ("torch.uint8", "torch.int64", "torch.uint8") and text.is_cuda and toff.is_cuda and status.is_cuda
    padded, lens, _ = v.encode_tensor(SENTS, width=6, pad_id=len(v))        # the pad id lies outside the list: skipped, it is not a bad id
    text, toff, status = v.decode_tensor(padded, skip=[len(v)])
    assert tensor_lines(text, toff) == [r.encode() for r in rendered] and status.cpu().tolist() == [0] * len(SENTS)
    text, toff, status = v.decode_tensor(padded)                            # ... and not skipped, it is one
    assert tensor_lines(text, toff) == [r.encode() for r in rendered] and status.cpu().tolist() == [1] * len(SENTS)
    assert v.decode([i.tolist() for i in v.encode(SENTS)]) == [r.encode() for r in rendered]
    v.close()


def test_round_trip_on_the_bert_like_list(small_env):
    w = small_env.words()
    v = w.vocabulary(LIST, 1, 2, 3, wordpiece=True)
    ids, off, _ = v.encode_tensor(["テストあいうえお", "形態素"])
    text, toff, status = v.decode_tensor(ids, off)                          # skip=None: the handle's bos and eos
    assert tensor_lines(text, toff) == ["テスト あいうえお".encode(), b"[UNK]"] and status.cpu().tolist() == [0, 0]
    text, toff, status = v.decode_tensor(ids, off, skip=[])
    assert tensor_lines(text, toff) == ["[CLS] テスト あいうえお [SEP]".encode(), b"[CLS] [UNK] [SEP]"]
    text, toff, status = v.decode_tensor(ids, off, separator="", skip=[2, 3, 1])
    assert tensor_lines(text, toff) == ["テストあいうえお".encode(), b""]
    v.close()


def test_cli_encode_then_decode_prints_what_wakati_prints(small_env, tmp_path):
    import io

    from kanpyo_amd import cli
    from kanpyo_amd.dictfile import DictFile, save_dict

    path, vocab = tmp_path / "t.dict", tmp_path / "vocab.txt"
    save_dict(DictFile(small_env.dict, small_env.known, small_env.unk), str(path))
    data = "".join(s + "\n" for s in SENTS * 3).encode()
    listed = sorted({x for r in small_env.words().render(SENTS) for x in r.split(" ") if x})
    vocab.write_bytes(b"".join(w.encode() + b"\n" for w in ["<unk>", "<s>"] + listed))

    def run(command, argv, stdin):
        out = io.BytesIO()
        rc = getattr(cli, command)(cli.parse_args([command, "-c", str(path)] + argv), io.BytesIO(stdin), out)
        return rc, out.getvalue()

    rc, want = run("wakati", [], data)
    assert rc == 0 and want.count(b"\n") == len(SENTS) * 3
    rc, ids = run("encode", ["--vocab", str(vocab), "--bos", "<s>"], data)
    assert rc == 0 and ids.startswith(b"1 ")
    rc, got = run("decode", ["--vocab", str(vocab), "--skip", "1", "--block-bytes", "40"], ids)      # several blocks of whole lines
    assert rc == 0 and got == want
    rc, got = run("decode", ["--vocab", str(vocab), "--separator", ""], ids)
    assert rc == 0 and got == b"".join(b"<s>" + ln.replace(b" ", b"") + b"\n" for ln in want.split(b"\n")[:-1])
    rc, got = run("decode", ["--vocab", str(vocab), "2 3 99"], b"")                                  # INPUT; an id outside the file gives nothing
    assert rc == 0 and got == (listed[0] + " " + listed[1]).encode() + b"\n"
    rc, got = run("decode", ["--vocab", str(vocab), "--block-bytes", "40"], ids + b"1 2 x\n")        # not a list of int32s: 101, and nothing on stdout
    assert rc == cli.PANIC_STATUS and got == b""


# ---- 4. the host call; the first-call upload ---------------------------------------------------------------------------------------------------------------
def test_host_call_equals_decode_tensor_two_threads_at_once(small_env, monkeypatch):
    import torch

    rng = random.Random(3)
    seqs = [[rng.randrange(-1, len(CRAFT)) for _ in range(rng.choice((0, 1, 5, 64, 65, 200)))] for _ in range(40)]
    want = R.decode(CRAFT, seqs, PREFIX, b" ", [])[0]
    v = small_env.words().vocabulary(CRAFT, 2, wordpiece=True)              # a fresh handle: the two threads race for its first decode
    got, errors = [None, None], []

    def run(k):
        try:
            got[k] = v.decode(seqs, skip=[])
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got[0] == got[1] == want
    flat = np.array([i for s in seqs for i in s], dtype=np.int32)
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    text, toff, _ = v.decode_tensor(torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), skip=[])
    assert tensor_lines(text, toff) == want
    monkeypatch.setenv("KGPU_HOST_CHUNK_SENTS", "7")                         # several chunks: the offsets run on, the capacity answer is exact
    assert v.decode(seqs, skip=[]) == want
    from kanpyo_amd.decode import host_call
    from functools import partial

    with pytest.raises(_lib.KgpuError) as e:
        host_call(partial(_lib.lib().kgpu_decode_batch, v.handle), flat, off.astype(np.uint64), 0, decode_opts(), text_capacity=sum(map(len, want)) - 1)
    assert e.value.code == _lib.KGPU_ERR_CAPACITY and e.value.bytes == sum(map(len, want))
    v.close()


def test_a_first_decode_leaves_the_handle_info_unchanged(small_env):
    v = small_env.words().vocabulary(LIST, 1, 2, 3, wordpiece=True)
    ids, off, _ = v.encode_tensor(["テスト"])
    before, wp_before, dict_before = v.info(), v.wordpiece_info(), small_env.tok.info()
    text, toff, _ = v.decode_tensor(ids, off)
    assert tensor_lines(text, toff) == ["テスト".encode()]
    assert v.info() == before and v.wordpiece_info() == wp_before and small_env.tok.info() == dict_before
    ids2, off2, _ = v.encode_tensor(["テスト"])
    assert ids2.cpu().tolist() == ids.cpu().tolist()                        # ... and it encodes as before
    v.close()
