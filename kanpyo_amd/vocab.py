"""Vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids"): sentences to int32 ids of a fixed word list, on the device.

A Vocab is made from a Words handle (Words.vocabulary, WordCounts.vocabulary, Vocab.load) and inherits its field and filter.  Every kept
token gives the index of its word in the list, or unk_id; a sentence's sequence is [bos] ids... [eos].  The host forms return numpy arrays
(ragged: ids + id_offsets); encode_tensor leaves everything in device memory as torch tensors, ragged -- the (input, offsets) pair
torch.nn.EmbeddingBag takes -- or padded to [n, width].
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import List, Sequence

import numpy as np

from . import _lib


def _word_bytes(w) -> bytes:
    return w.encode("utf-8") if isinstance(w, str) else bytes(w)


class Vocab:
    """A vocabulary handle (kgpu_vocab): a frozen word -> id table on the device.  Immutable; usable from many threads at once; it keeps its
    Words handle's tables and the dictionary alive and may outlive both (encode_tensor alone needs the Tokenizer open).  .words is the list (bytes), id k is words[k]."""

    def __init__(self, words_handle, words: Sequence, unk_id: int, bos_id=None, eos_id=None):
        from .tokenizer import pack_sentences

        self.words = [_word_bytes(w) for w in words]
        self.unk_id, self.bos_id, self.eos_id = int(unk_id), bos_id, eos_id
        flags = (_lib.KGPU_VOCAB_ADD_BOS if bos_id is not None else 0) | (_lib.KGPU_VOCAB_ADD_EOS if eos_id is not None else 0)
        packed, offs = pack_sentences(self.words)
        packed = np.ascontiguousarray(packed)
        opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), flags, int(unk_id), int(bos_id or 0), int(eos_id or 0))
        h = C.c_void_p()
        _lib.check(_lib.lib().kgpu_vocab_create(words_handle.handle, packed.ctypes.data if packed.size else None, offs.ctypes.data, len(self.words),
                                                C.byref(opts), C.byref(h)))
        self._h = h
        self._tokenizer = words_handle.tokenizer   # (encode_tensor's context is made from it)
        self._device = self._tokenizer.info()["device"]
        self._extra = (1 if bos_id is not None else 0) + (1 if eos_id is not None else 0)
        self._ctx = None
        self._ctx_lock = threading.Lock()

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_ctx", None) is not None:
            self._ctx.close()
            self._ctx = None
        if getattr(self, "_h", None):
            _lib.lib().kgpu_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.words)

    def info(self) -> dict:
        """kgpu_vocab_get_info: n_words, table_slots, key_bytes, rows_resolved."""
        i = _lib.VocabInfo(C.sizeof(_lib.VocabInfo))
        _lib.check(_lib.lib().kgpu_vocab_get_info(self._h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_ if n not in ("size", "reserved")}

    # ---- host memory in and out ------------------------------------------------------------------------------------------------------------
    def encode_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None):
        """kgpu_encode_batch -> (ids[int32], id_offsets[uint64 n+1], status[uint8 n]): sentence i's sequence is
        ids[id_offsets[i]:id_offsets[i+1]].  out=(ids, id_offsets, status): caller-owned arrays to reuse (too small: KgpuError with
        KGPU_ERR_CAPACITY, nothing written)."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        total = int(offsets[-1] - offsets[0]) if n else 0
        cap = total // 2 + n * (1 + self._extra) + 64
        L = _lib.lib()
        while True:
            if out is not None:
                ids, ioff, status = out
                if ids.dtype != np.int32 or ioff.dtype != np.uint64 or status.dtype != np.uint8 or ioff.size < n + 1 or status.size < n:
                    raise ValueError("out=(ids[int32], id_offsets[uint64 >= n+1], status[uint8 >= n])")
                cap = ids.size
            else:
                ids = np.empty(max(cap, 1), dtype=np.int32)
                ioff = np.empty(n + 1, dtype=np.uint64)
                status = np.empty(max(n, 1), dtype=np.uint8)
            status[: max(n, 1)] = 0
            got = C.c_uint64(0)
            rc = L.kgpu_encode_batch(self._h, utf8.ctypes.data if utf8.size else None, offsets.ctypes.data, n, ids.ctypes.data, cap, ioff.ctypes.data,
                                     status.ctypes.data, C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and out is None:
                cap = int(got.value)   # the exact count reported by the device
                continue
            _lib.check(rc)
            return ids[: int(got.value)], ioff[: n + 1], status[:n]

    def encode_text(self, block):
        """kgpu_encode_text: a raw block of input (bytes or uint8 array) -> (ids, id_offsets, status) as encode_packed(*split_lines(block))
        gives them; the split and the trim run on the device."""
        from .tokenizer import _block_bytes

        src = _block_bytes(block)
        cap, ocap = src.size // 2 + 64, src.size // 16 + 1024
        cap += ocap * self._extra
        L = _lib.lib()
        while True:
            ids = np.empty(max(cap, 1), dtype=np.int32)
            ioff = np.empty(ocap, dtype=np.uint64)
            status = np.zeros(ocap, dtype=np.uint8)
            n, got = C.c_uint64(0), C.c_uint64(0)
            rc = L.kgpu_encode_text(self._h, src.ctypes.data if src.size else None, src.size, ids.ctypes.data, cap, ioff.ctypes.data, ocap,
                                    status.ctypes.data, C.byref(n), C.byref(got))
            if rc == _lib.KGPU_ERR_CAPACITY and (int(got.value) > cap or int(n.value) + 1 > ocap):   # exact sizes reported by the device
                cap, ocap = max(cap, int(got.value)), max(ocap, int(n.value) + 1)
                continue
            _lib.check(rc)
            k = int(n.value)
            return ids[: int(got.value)], ioff[: k + 1], status[:k]

    def encode(self, sentences: Sequence) -> List[np.ndarray]:
        """One int32 array per sentence (str or bytes)."""
        from .tokenizer import pack_sentences

        ids, ioff, _ = self.encode_packed(*pack_sentences(sentences))
        o = ioff.tolist()
        return [ids[o[i] : o[i + 1]] for i in range(len(o) - 1)]

    # ---- device memory out -----------------------------------------------------------------------------------------------------------------
    def encode_tensor(self, sentences: Sequence, width=None, pad_id: int = 0):
        """The sentences (str or bytes) as torch tensors on the device, in ONE DeviceContext batch: upload, tokenize, sync, encode, sync_lines.
        No id passes through host memory.  THE WHOLE BATCH MUST FIT DEVICE MEMORY (its text, 24 bytes per token and 4 bytes per id): cut a
        corpus into batches.  The batch is tokenized on a DeviceContext of this Vocab's Tokenizer, made by the first call: unlike the host
        forms, which work on a Vocab that has outlived its Words and its Tokenizer, encode_tensor NEEDS THE TOKENIZER OPEN (RuntimeError otherwise).
        width=None -> (ids int32 [total], offsets int64 [n + 1], status uint8 [n]); ids and offsets[:-1] are what torch.nn.EmbeddingBag takes.
        width=w    -> (ids int32 [n, w], lengths int64 [n] = min(L, w), status uint8 [n]); rows are cut after w elements (a cut row ends with
        eos_id when the vocabulary adds EOS) and filled with pad_id."""
        import torch

        from .device import DeviceContext
        from .tokenizer import pack_sentences

        if width is not None and int(width) < 1:
            raise ValueError("width is 1 or more (None: ragged)")
        utf8, offs = pack_sentences(sentences)
        n, total = offs.size - 1, int(offs[-1])
        with self._ctx_lock:
            if self._ctx is None:
                if not getattr(self._tokenizer, "_h", None):
                    raise RuntimeError("encode_tensor tokenizes on a context of the Vocab's Tokenizer, which has been closed; encode_packed / encode_text still work")
                self._ctx = DeviceContext(self._tokenizer)
            ctx = self._ctx
            dev = torch.device("cuda", self._device)
            d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_st = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
            cap = total // 2 + n + 64
            L = _lib.lib()
            while True:   # (a token buffer too small: once more with the count the device reports, as tokenize_packed does)
                d_tok = torch.empty((cap, 6), dtype=torch.int32, device=dev)
                torch.cuda.synchronize(dev)
                ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, total, d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr())
                got = C.c_uint64(0)
                rc = L.kgpu_ctx_sync(ctx._h, C.byref(got))
                if rc == _lib.KGPU_ERR_CAPACITY and int(got.value) > cap:
                    cap = int(got.value) + 64
                    continue
                _lib.check(rc)
                break
            n_tok = int(got.value)
            d_ioff = torch.empty(n + 1, dtype=torch.int64, device=dev)
            if width is None:
                id_cap = n_tok + n * self._extra   # (every record kept, and bos / eos: never too small)
                d_ids = torch.empty(max(id_cap, 1), dtype=torch.int32, device=dev)
            else:
                id_cap = n * int(width)
                d_ids = torch.empty((n, int(width)), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            ctx.encode(self, d_utf8.data_ptr(), d_off.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), d_ids.data_ptr(), id_cap, d_ioff.data_ptr(),
                       width=0 if width is None else int(width), pad_id=int(pad_id))
            count = ctx.sync_lines()
        if width is None:
            return d_ids[:count], d_ioff, d_st[:n]
        return d_ids, torch.clamp(d_ioff[1:] - d_ioff[:-1], max=int(width)), d_st[:n]

    # ---- the one-word-per-line file ----------------------------------------------------------------------------------------------------------
    def save(self, path):
        """One word per line, as raw bytes: line k (0-based) is id k.  ValueError: a word holds a newline."""
        for k, w in enumerate(self.words):
            if b"\n" in w:
                raise ValueError(f"word {k} holds a newline: the one-word-per-line file cannot say it")
        with open(path, "wb") as f:
            f.write(b"".join(w + b"\n" for w in self.words))

    @staticmethod
    def read_words(path) -> List[bytes]:
        """The list of a file written by save (or by `count ... | cut -f2`): every '\\n'-terminated line is a word, the empty line the empty word."""
        with open(path, "rb") as f:
            data = f.read()
        lines = data.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        return lines

    @classmethod
    def load(cls, words_handle, path, unk="<unk>", bos=None, eos=None) -> "Vocab":
        """A Vocab over the file's list.  unk, bos, eos: WORDS that must be in the file (ValueError otherwise); bos / eos None: not added."""
        return cls.from_words(words_handle, cls.read_words(path), unk, bos, eos)

    @classmethod
    def from_words(cls, words_handle, words: Sequence, unk="<unk>", bos=None, eos=None) -> "Vocab":
        """A Vocab whose unk / bos / eos ids are the list indices of those words."""
        words = [_word_bytes(w) for w in words]
        index = {}
        for k, w in enumerate(words):
            index.setdefault(w, k)
        ids = []
        for what, w in (("unk", unk), ("bos", bos), ("eos", eos)):
            if w is None:
                ids.append(None)
                continue
            b = _word_bytes(w)
            if b not in index:
                raise ValueError(f"the {what} word {b!r} is not in the vocabulary")
            ids.append(index[b])
        return cls(words_handle, words, ids[0], ids[1], ids[2])
