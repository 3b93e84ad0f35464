"""The host side of the `kanpyo tokenize` output (src/bin/kanpyo.rs:106-126, 174-197), without a device: the bincode parser, validation
and joined pool behind kgpu_dict_set_features (through the kgpu_debug_feature_pool hook) against MorphFeatureTable's own codec;
kgpu_split_lines against a restatement of read_line + str::trim_end; the C consumer of the lines entry points; the CLI's error path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from kanpyo_amd import _lib
from kanpyo_amd.dictfile import MorphFeatureTable, enc_varint
from kanpyo_amd.tokenizer import split_lines

# char::is_whitespace: the Unicode White_Space property, 25 code points
WHITE_SPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680" + "".join(map(chr, range(0x2000, 0x200B))) + "\u2028\u2029\u202f\u205f\u3000"
assert len(WHITE_SPACE) == 25


def _pool(known: bytes, unk: bytes, n_morphs: int, n_unk: int):
    L = _lib.lib()
    off = np.zeros(n_morphs + n_unk + 1, dtype=np.uint32)
    got = C.c_uint64(0)
    a, b = np.frombuffer(known, dtype=np.uint8), np.frombuffer(unk, dtype=np.uint8)
    args = (a.ctypes.data if a.size else None, a.size, b.ctypes.data if b.size else None, b.size, n_morphs, n_unk)
    rc = L.kgpu_debug_feature_pool(*args, None, 0, off.ctypes.data, C.byref(got))
    if rc != _lib.KGPU_ERR_CAPACITY or got.value == 0:
        return rc, None, None
    pool = np.zeros(got.value, dtype=np.uint8)
    rc = L.kgpu_debug_feature_pool(*args, pool.ctypes.data, pool.size, off.ctypes.data, C.byref(got))
    return rc, pool.tobytes(), off


def _expected(known: MorphFeatureTable, unk: MorphFeatureTable, n_morphs: int, n_unk: int):
    rows = [",".join(known.features(i)).encode() for i in range(1, n_morphs + 1)]
    rows += [",".join(unk.features(i)).encode() for i in range(1, n_unk + 1)]
    return b"".join(rows), np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)


def _draw_table(rng, n_rows, n_names, long_names=False):
    names = [""]
    for i in range(1, n_names):
        k = int(rng.integers(0, 4))
        s = ["名詞", "ｶﾀｶﾅ", "*", "x"][k] + str(i)
        if long_names and i % 97 == 0:
            s = "長" * int(rng.integers(84, 200))   # 252..600 bytes: a 3-byte length varint
        names.append(s)
    rows = []
    for r in range(n_rows):
        k = int(rng.integers(0, 10))
        if r % 17 == 0:
            k = 0                                    # an empty row
        ids = rng.integers(0, n_names, size=k).tolist()
        if r % 29 == 0:
            ids.append(0)                            # name_list[0] == "": an empty field
        if r % 13 == 0:
            ids.append(n_names - 1)                  # the largest id
        rows.append(ids)
    return MorphFeatureTable(rows, names)


@pytest.mark.parametrize("n_names", [40, 300, 70000])
def test_pool_matches_the_python_codec(n_names):
    rng = np.random.default_rng(n_names)
    known = _draw_table(rng, 500, n_names, long_names=True)
    unk = _draw_table(rng, 40, min(n_names, 300))
    for n_morphs, n_unk in ((500, 40), (321, 7), (0, 0)):
        rc, pool, off = _pool(known.encode(), unk.encode(), n_morphs, n_unk)
        want, want_off = _expected(known, unk, n_morphs, n_unk)
        if not want:
            assert rc == _lib.KGPU_OK
            continue
        assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
        assert pool == want and np.array_equal(off, want_off)
    # trailing bytes are ignored (decode_from_slice)
    rc, pool, _ = _pool(known.encode() + b"\xff\x00junk", unk.encode() + b"\x01", 500, 40)
    assert rc == _lib.KGPU_OK and pool == _expected(known, unk, 500, 40)[0]


def test_varint_widths_1_3_5_and_9_bytes():
    names = ["", "a" * 300, "é"] + [f"n{i}" for i in range(3, 65540)]
    t = MorphFeatureTable([[1, 2], [65539, 251, 0], []], names)
    enc = t.encode()
    assert enc_varint(300) in enc and enc_varint(65539) in enc and enc_varint(251) in enc   # 3-byte length, 5- and 3-byte ids
    # the same table with every length written as a 9-byte varint (tag 253 + u64): bincode reads it the same
    wide = lambda v: b"\xfd" + v.to_bytes(8, "little")  # noqa: E731
    parts = [wide(len(t.morph_features))]
    for row in t.morph_features:
        parts.append(wide(len(row)) + b"".join(enc_varint(x) for x in row))
    parts.append(wide(len(names)))
    parts += [wide(len(s.encode())) + s.encode() for s in names]
    for blob in (enc, b"".join(parts)):
        rc, pool, off = _pool(blob, MorphFeatureTable([], [""]).encode(), 3, 0)
        assert rc == _lib.KGPU_OK
        assert pool == ("a" * 300 + ",é" + "n65539,n251,").encode()
        assert off.tolist() == [0, 303, 303 + 12, 303 + 12]


def _rc(known: bytes, unk: bytes, n_morphs=2, n_unk=1):
    rc, _, _ = _pool(known, unk, n_morphs, n_unk)
    return rc, _lib.lib().kgpu_last_error().decode()


def test_rejections():
    ok_k = MorphFeatureTable([[1, 2], [2]], ["", "a", "b"])
    ok_u = MorphFeatureTable([[1]], ["", "u"])
    assert _rc(ok_k.encode(), ok_u.encode())[0] == _lib.KGPU_OK
    # fewer rows than morphs / unknown morphs: morph_features[id - 1] would panic (kanpyo.rs:178-186)
    rc, msg = _rc(ok_k.encode(), ok_u.encode(), n_morphs=3)
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:178-186" in msg
    rc, msg = _rc(ok_k.encode(), ok_u.encode(), n_unk=2)
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:178-186" in msg
    # a feature id at or past name_list.len() (:181 known, :188 unknown)
    rc, msg = _rc(MorphFeatureTable([[1], [3]], ["", "a", "b"]).encode(), ok_u.encode())
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:181" in msg
    rc, msg = _rc(ok_k.encode(), MorphFeatureTable([[2]], ["", "u"]).encode())
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:188" in msg
    # every truncation of either blob
    for blob in (ok_k.encode(), ok_u.encode()):
        for cut in range(len(blob)):
            k = blob[:cut] if blob == ok_k.encode() else ok_k.encode()
            u = blob[:cut] if blob != ok_k.encode() else ok_u.encode()
            rc, msg = _rc(k, u)
            assert rc == _lib.KGPU_ERR_BAD_DICT and "truncated" in msg, (cut, msg)
    # varint tag 255; an id tag wider than u32; a name that is not UTF-8
    assert _rc(b"\xff", ok_u.encode())[0] == _lib.KGPU_ERR_BAD_DICT
    assert _rc(b"\x01\x01\xfd" + (1).to_bytes(8, "little") + b"\x02\x00\x01a", ok_u.encode(), n_morphs=1)[0] == _lib.KGPU_ERR_BAD_DICT
    for bad in (b"\xff", b"\xc0\x80", b"\xed\xa0\x80", b"\xe3\x80", b"\xf4\x90\x80\x80"):
        blob = b"\x01\x01\x01\x02\x00" + enc_varint(len(bad)) + bad
        rc, msg = _rc(blob, ok_u.encode(), n_morphs=1)
        assert rc == _lib.KGPU_ERR_BAD_DICT and "UTF-8" in msg, bad
    assert _rc(b"\x01\x01\x01\x02\x00\x03\xe3\x80\x80", ok_u.encode(), n_morphs=1)[0] == _lib.KGPU_OK   # U+3000 is fine


# ---- kgpu_split_lines -----------------------------------------------------------------------------------------------------
def _ref_split(b: bytes):
    """read_line (up to and including '\\n'; the last line may lack it) + trim_end; invalid bytes are never White_Space."""
    if not b:
        return []
    parts = b.split(b"\n")
    if b.endswith(b"\n"):
        parts.pop()
    return [p.decode("utf-8", "surrogateescape").rstrip(WHITE_SPACE).encode("utf-8", "surrogateescape") for p in parts]


def _split(b: bytes):
    text, offs = split_lines(b)
    t = text.tobytes()
    return [t[int(offs[i]) : int(offs[i + 1])] for i in range(len(offs) - 1)]


def test_split_lines_cases():
    assert _split(b"") == []
    assert _split(b"\n") == [b""]
    assert _split(b"a") == [b"a"] and _split(b"a\n") == [b"a"] and _split(b"a\n\n") == [b"a", b""]
    assert _split("すもも\r\nもも \u3000\n  \t\nlast".encode()) == ["すもも".encode(), "もも".encode(), b"", b"last"]
    for ws in WHITE_SPACE.replace("\n", ""):
        assert _split(("x" + ws + ws + "\n").encode()) == [b"x"], hex(ord(ws))
        assert _split((ws + "x").encode()) == [(ws + "x").encode()]          # leading space is kept
    for keep in "\x1c\x1d\x1e\x1f\u200b\ufeff\x00":
        assert _split(("x" + keep).encode()) == [("x" + keep).encode()], hex(ord(keep))
    # invalid bytes before and inside trailing space: only complete encodings go
    assert _split(b"x\xff \xe3\x80\x80") == [b"x\xff"]
    assert _split(b"x\xe3\x80") == [b"x\xe3\x80"]            # a truncated U+3000 stays
    assert _split(b"x\xe3\xe3\x80\x80") == [b"x\xe3"]
    assert _split(b"x\xc2 \xc2\x85") == [b"x\xc2"]
    assert _split(b"\x80\x20") == [b"\x80"]


def test_split_lines_drawn_against_the_restatement():
    rng = np.random.default_rng(5)
    alphabet = [c.encode() for c in WHITE_SPACE + "\x1c\x1d\x1e\x1fa\u3042\u6f22\u200b"] + [b"\xff", b"\xe3", b"\x80", b"\xc2", b"\xe2\x80", b"\r\n"]
    for _ in range(3000):
        b = b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 30))))
        assert _split(b) == _ref_split(b), b


def test_split_lines_capacity():
    L = _lib.lib()
    src = b"a\nb\nc"
    out = np.zeros(8, dtype=np.uint8)
    offs = np.zeros(3, dtype=np.uint64)
    n = C.c_uint64(0)
    assert L.kgpu_split_lines(src, len(src), out.ctypes.data, offs.ctypes.data, 3, C.byref(n)) == _lib.KGPU_ERR_CAPACITY and n.value == 3
    offs = np.zeros(4, dtype=np.uint64)
    assert L.kgpu_split_lines(src, len(src), out.ctypes.data, offs.ctypes.data, 4, C.byref(n)) == _lib.KGPU_OK
    assert offs.tolist() == [0, 1, 2, 3] and out[:3].tobytes() == b"abc"


# ---- the C consumer and the CLI ---------------------------------------------------------------------------------------------
def test_lines_consumer_is_strict_c99_and_links(tmp_path):
    exe = str(tmp_path / "lines_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "lines_consumer.c"), "-o", exe, "-L", libdir, "-lkanpyo_gpu", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(exe)


def test_new_symbols_are_exported():
    L = _lib.lib()
    for s in ("kgpu_dict_set_features", "kgpu_tokenize_batch_lines", "kgpu_format_lines_device", "kgpu_ctx_sync_lines", "kgpu_split_lines"):
        assert s in _lib.SYMBOLS and hasattr(L, s)


def test_cli_without_a_device(tmp_path, fixture_dict):
    from kanpyo_amd.dictfile import DictFile, save_dict

    path = tmp_path / "t.dict"
    save_dict(DictFile(fixture_dict, MorphFeatureTable([[1]] * fixture_dict.n_morphs, ["", "f"]), MorphFeatureTable([[1]] * 8, ["", "u"])), str(path))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "kanpyo_amd", "tokenize", "-c", str(path)], input=b"abc\n", capture_output=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode != 0 and r.stdout == b""
    assert f"kgpu error {_lib.KGPU_ERR_NO_DEVICE}" in r.stderr.decode(), r.stderr.decode()
