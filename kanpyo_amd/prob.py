"""Lattice probabilities (include/kanpyo_gpu.h, "lattice probabilities"): the lattice read as a distribution over tokenizations, P(path) proportional
to exp(-theta cost) -- token marginals (what `mecab -m` gives) and sampled paths (`mecab -l --theta`).  marginals_host and samples_host are the rule on
the host (a Lattice in, numpy out, no device): what Tokenizer.tokenize_marginals_packed / tokenize_samples_packed compute on the device is defined by
them, byte for byte."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._calls import TOKEN_DTYPE, grown
from .nbest import connection_matrix, lattice_struct

THETA_DEFAULT = _lib.KGPU_THETA_DEFAULT   # MeCab's default theta, 0.75, over IPADIC's cost factor, 800


def kexp_host(x) -> np.ndarray:
    """The rule's exp over an array of doubles <= 0 (kgpu_prob_exp_host)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    _lib.lib().kgpu_prob_exp_host(x.ctypes.data, x.size, out.ctypes.data)
    return out


def klog_host(x) -> np.ndarray:
    """The rule's log over an array of positive normal doubles (kgpu_prob_log_host)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    _lib.lib().kgpu_prob_log_host(x.ctypes.data, x.size, out.ctypes.data)
    return out


def marginals_host(lattice, connection, theta: float = THETA_DEFAULT, all_nodes: bool = False, min_prob: float = 0.0) -> tuple:
    """kgpu_marginals_host -> (tokens[TOKEN_DTYPE], probs[float64], on_best[uint8], log_z, best_logprob): the records of tokenize's path with their
    marginals (EOS last, with 1), or with all_nodes every node but BOS whose marginal is at least min_prob, in node order.  connection: see
    nbest.connection_matrix.  Needs no device."""
    lat, keep = lattice_struct(lattice)
    conn, rows, cols = connection_matrix(connection)
    caps = (len(lattice.nodes),)
    T, lz, bl = C.c_uint64(0), C.c_double(0), C.c_double(0)
    while caps is not None:
        tokens, probs, best = np.zeros(max(caps[0], 1), dtype=TOKEN_DTYPE), np.zeros(max(caps[0], 1), dtype=np.float64), np.zeros(max(caps[0], 1), dtype=np.uint8)
        rc = _lib.lib().kgpu_marginals_host(C.byref(lat), conn.ctypes.data, rows, cols, float(theta), _lib.KGPU_MARGINAL_ALL if all_nodes else _lib.KGPU_MARGINAL_BEST,
                                            float(min_prob), tokens.ctypes.data, caps[0], probs.ctypes.data, best.ctypes.data, C.byref(lz), C.byref(bl), C.byref(T))
        caps = grown(rc, caps, (T.value,))
    del keep
    return tokens[: T.value], probs[: T.value], best[: T.value], lz.value, bl.value


def samples_host(lattice, connection, n_samples: int, seed: int = 0, sentence_index: int = 0, theta: float = THETA_DEFAULT) -> tuple:
    """kgpu_samples_host -> (tokens[TOKEN_DTYPE], tok_offsets[uint64 P + 1], costs[int32 P]): n_samples paths drawn from the lattice (none where EOS is
    unreachable), N-best's format.  sentence_index: the sentence's index in the device call this stands for.  Needs no device."""
    lat, keep = lattice_struct(lattice)
    conn, rows, cols = connection_matrix(connection)
    caps = (len(lattice.nodes) * max(min(int(n_samples), 4), 1), max(int(n_samples), 0))
    P, T = C.c_uint64(0), C.c_uint64(0)
    while caps is not None:
        tokens, toff, costs = np.zeros(max(caps[0], 1), dtype=TOKEN_DTYPE), np.zeros(caps[1] + 1, dtype=np.uint64), np.zeros(max(caps[1], 1), dtype=np.int32)
        rc = _lib.lib().kgpu_samples_host(C.byref(lat), conn.ctypes.data, rows, cols, float(theta), int(n_samples), int(seed) & (2**64 - 1), int(sentence_index),
                                          tokens.ctypes.data, caps[0], toff.ctypes.data, costs.ctypes.data, caps[1], C.byref(P), C.byref(T))
        caps = grown(rc, caps, (T.value, P.value))
    del keep
    return tokens[: T.value], toff[: P.value + 1], costs[: P.value]


def marginal_lines(raw: bytes, tokens, probs, known, unk) -> bytes:
    """The `kanpyo tokenize` lines of these records, each with `\\t%.6f` -- its marginal -- appended (nbest.path_lines with one more column)."""
    from .nbest import path_lines

    lines = path_lines(raw, tokens, known, unk).split(b"\n")[:-1]
    return b"".join(line + b"\t%.6f\n" % float(p) for line, p in zip(lines, probs))
