"""N-best paths (include/kanpyo_gpu.h, "N-best paths"): the k lowest-cost tokenizations of a sentence, what `mecab -N k` prints.  nbest_host is the
rule on the host (a Lattice in, numpy out, no device): what Tokenizer.tokenize_nbest_packed computes on the device is defined by it.  path_lines
renders paths as the `kanpyo tokenize` lines of their records, on the host."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib
from ._calls import TOKEN_DTYPE, grown


def connection_matrix(connection) -> tuple:
    """The connection matrix in whichever form -> (int16 array, rows, cols), element (right_id, left_id) at left_id * rows + right_id: a Dict (its
    connection_dict), the connection.dict blob itself (connection.rs:44-51: rows, cols as u64, then the int16s), or (values, rows, cols) -- what this function returns."""
    blob = getattr(connection, "connection_dict", connection)
    if isinstance(blob, (bytes, bytearray, memoryview)):
        blob = bytes(blob)
        rows, cols = struct.unpack_from("<QQ", blob, 0)
        data = np.frombuffer(blob, dtype="<i2", offset=16)
    else:
        data, rows, cols = blob
        data = np.ascontiguousarray(data, dtype=np.int16).reshape(-1)
    if data.size < rows * cols:
        raise ValueError("the connection matrix holds fewer values than rows x cols")
    return np.ascontiguousarray(data[: rows * cols]), int(rows), int(cols)


def lattice_struct(lattice) -> tuple:
    """A kanpyo_amd.lattice.Lattice as the kgpu_lattice kgpu_lattice_dump returns -> (_lib.LatticeOut, the arrays it points into)."""
    nodes = (_lib.LatticeNode * max(len(lattice.nodes), 1))()
    i16 = lambda v: ((int(v) + 0x8000) & 0xFFFF) - 0x8000   # noqa: E731  (a context id of 32768 and more, as the dump's int16 holds it)
    for k, n in enumerate(lattice.nodes):
        nodes[k] = _lib.LatticeNode(n.id, int(n.class_), n.byte_pos, n.char_pos, n.end_char, len(n.surface.encode("utf-8")), i16(n.left_id), i16(n.right_id),
                                    i16(n.cost), 0, n.dp, -1 if n.pre is None else n.pre)
    eo = np.zeros(len(lattice.edges) + 1, dtype=np.uint32)
    if lattice.edges:
        eo[1:] = np.cumsum([len(e) for e in lattice.edges])
    en = np.array([j for e in lattice.edges for j in e] or [0], dtype=np.uint32)
    out = _lib.LatticeOut(len(lattice.nodes), len(lattice.edges), nodes, eo.ctypes.data_as(C.POINTER(C.c_uint32)), en.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out, (nodes, eo, en)


def nbest_host(lattice, connection, n_best: int) -> tuple:
    """kgpu_nbest_host -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 P + 1], costs[int32 P]): the P <= n_best lowest-cost paths of the lattice, best
    first; path p's records are tokens[tok_offsets[p]:tok_offsets[p + 1]].  connection: see connection_matrix.  Needs no device."""
    lat, keep = lattice_struct(lattice)
    conn, rows, cols = connection_matrix(connection)
    caps = (len(lattice.nodes), max(int(n_best), 0))   # (grown to the exact sizes where the paths hold more records than the lattice has nodes)
    P, T = C.c_uint64(0), C.c_uint64(0)
    while caps is not None:
        tokens, toff, costs = np.zeros(max(caps[0], 1), dtype=TOKEN_DTYPE), np.zeros(caps[1] + 1, dtype=np.uint64), np.zeros(max(caps[1], 1), dtype=np.int32)
        rc = _lib.lib().kgpu_nbest_host(C.byref(lat), conn.ctypes.data, rows, cols, int(n_best), tokens.ctypes.data, caps[0], toff.ctypes.data, costs.ctypes.data,
                                        caps[1], C.byref(P), C.byref(T))
        caps = grown(rc, caps, (T.value, P.value))
    del keep
    return tokens[: T.value], toff[: P.value + 1], costs[: P.value]


def path_lines(raw: bytes, tokens, known, unk) -> bytes:
    """The `surface\\tfeatures` lines of one path's records (reference src/bin/kanpyo.rs:174-197: print_tokens), its EOS line last.  raw: the
    sentence's bytes; known / unk: the display tables (anything with .features(id))."""
    out = []
    for t in tokens:
        cls, tid, pos, bl = int(t["cls"]), int(t["id"]), int(t["position"]), int(t["byte_len"])
        feats = ",".join((known if cls == 1 else unk).features(tid)).encode("utf-8") if cls != 0 and tid != 0 else b""
        out.append((b"EOS" if cls == 0 else raw[pos : pos + bl]) + b"\t" + feats + b"\n")
    return b"".join(out)
