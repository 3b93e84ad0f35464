"""Vocabulary ids (include/kanpyo_gpu.h, "vocabulary ids"): sentences to int32 ids of a fixed word list, on the device.

A Vocab is made from a Words handle (Words.vocabulary, WordCounts.vocabulary, Vocab.load) and inherits its field and filter.  Every kept
token gives the index of its word in the list, or unk_id; a sentence's sequence is [bos] ids... [eos].  The host forms return numpy arrays
(ragged: ids + id_offsets); encode_tensor leaves everything in device memory as torch tensors, ragged -- the (input, offsets) pair
torch.nn.EmbeddingBag takes -- or padded to [n, width].

wordpiece=True (include/kanpyo_gpu.h, "WordPiece ids"): the list is a BERT vocab.txt -- a word outside it is cut greedily into its longest listed
pieces, continuation pieces listed behind the prefix ("##"), and a kept token gives zero, one or many ids.  What is pinned is that split rule, not
equal input_ids with a real BERT-Japanese tokenizer (its NFKC is available -- Tokenizer.words(normalize="NFKC") -- but it segments with the real IPADIC).

A Vocab made from a Words handle with normalize="NFC" / "NFKC" normalises the input of every encode call on the device first; the ids are those of
the NORMALISED text, and a status byte is 4 where the normaliser left a line as it was.  Unlike the plain host forms, that needs the Tokenizer open.

Ids with spans (include/kanpyo_gpu.h, "ids with spans"): encode_tensor(return_spans=True) and encode_spans give, beside every id, its span in the text
the caller supplied (through the normaliser's edit records when a form is set) and the index of its token -- an offset_mapping and word_ids().
"""
from __future__ import annotations

import ctypes as C
import threading
from functools import partial
from typing import List, Sequence

import numpy as np

from . import _lib
from ._calls import SPAN_DTYPE, Handle, batch_call, block_call, device_call, pack_sentences, ptr, struct_dict
from .device import DeviceContext


def _word_bytes(w) -> bytes:
    return w.encode("utf-8") if isinstance(w, str) else bytes(w)


def _stage(dev, alloc, enqueue, wait, caps: tuple, slack: int = 0, fixed: bool = False) -> tuple:
    """One stage of encode_tensor / encode_pairs_tensor over device_call.  An attempt: alloc(*caps) -> the buffers the capacities size, ONE
    torch.cuda.synchronize (they are ready before the library's stream uses them), enqueue(buffers, *caps), wait() -> (fits, sizes...).
    -> (sizes, buffers) of the attempt that fitted."""
    import torch

    def attempt(*caps):
        made = alloc(*caps)
        torch.cuda.synchronize(dev)
        enqueue(made, *caps)
        fits, *reported = wait()
        return _lib.KGPU_OK if fits else _lib.KGPU_ERR_CAPACITY, reported, made

    return device_call(attempt, caps, slack, fixed)


def wordpiece_opts(prefix="##", max_word_chars=100) -> "_lib.WordpieceOpts":
    """kgpu_wordpiece_opts of a prefix (str or bytes, at most 8 bytes) and a character limit (1..1024); ValueError otherwise."""
    p = _word_bytes(prefix)
    if len(p) > 8:
        raise ValueError(f"the prefix {p!r} has more than 8 bytes")
    if not 1 <= int(max_word_chars) <= 1024:
        raise ValueError("max_word_chars is 1..1024")
    return _lib.WordpieceOpts(C.sizeof(_lib.WordpieceOpts), int(max_word_chars), len(p), (C.c_uint8 * 8)(*p))


class Vocab(Handle):
    """A vocabulary handle (kgpu_vocab): a frozen word -> id table on the device.  Immutable; usable from many threads at once; it keeps its
    Words handle's tables and the dictionary alive and may outlive both (encode_tensor alone needs the Tokenizer open).  .words is the list (bytes), id k is words[k]."""

    _destroy = "kgpu_vocab_destroy"
    _ctx = None   # encode_tensor's DeviceContext, made by its first call

    def __init__(self, words_handle, words: Sequence, unk_id: int, bos_id=None, eos_id=None, wordpiece=False, prefix="##", max_word_chars=100):
        self.words = [_word_bytes(w) for w in words]
        self.wordpiece = bool(wordpiece)
        self._wp = wordpiece_opts(prefix, max_word_chars) if wordpiece else None
        self.unk_id, self.bos_id, self.eos_id = int(unk_id), bos_id, eos_id
        flags = (_lib.KGPU_VOCAB_ADD_BOS if bos_id is not None else 0) | (_lib.KGPU_VOCAB_ADD_EOS if eos_id is not None else 0)
        packed, offs = pack_sentences(self.words)
        packed = np.ascontiguousarray(packed)
        opts = _lib.VocabOpts(C.sizeof(_lib.VocabOpts), flags, int(unk_id), int(bos_id or 0), int(eos_id or 0))
        h = C.c_void_p()
        if wordpiece:
            _lib.check(_lib.lib().kgpu_vocab_create_wordpiece(words_handle.handle, ptr(packed), offs.ctypes.data, len(self.words),
                                                              C.byref(opts), C.byref(self._wp), C.byref(h)))
        else:
            _lib.check(_lib.lib().kgpu_vocab_create(words_handle.handle, ptr(packed), offs.ctypes.data, len(self.words),
                                                    C.byref(opts), C.byref(h)))
        self._h = h
        self._tokenizer = words_handle.tokenizer   # (encode_tensor's context is made from it)
        self._normalize = getattr(words_handle, "normalize", None)   # the form the encode calls normalise their input with first
        self._device = self._tokenizer.info()["device"]
        self._extra = (1 if bos_id is not None else 0) + (1 if eos_id is not None else 0)
        self._ctx_lock = threading.Lock()

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        super().close()

    def __len__(self):
        return len(self.words)

    def info(self) -> dict:
        """kgpu_vocab_get_info: n_words, table_slots, key_bytes, rows_resolved."""
        i = _lib.VocabInfo(C.sizeof(_lib.VocabInfo))
        _lib.check(_lib.lib().kgpu_vocab_get_info(self._h, C.byref(i)))
        return struct_dict(i)

    def wordpiece_info(self) -> dict:
        """kgpu_vocab_get_wordpiece_info: the continuation table, the row outcomes, the pool (KgpuError on a plain Vocab)."""
        i = _lib.WordpieceInfo(C.sizeof(_lib.WordpieceInfo))
        _lib.check(_lib.lib().kgpu_vocab_get_wordpiece_info(self._h, C.byref(i)))
        return struct_dict(i)

    def split_words(self, words: Sequence) -> List[np.ndarray]:
        """The split of each word (str or bytes) by this WordPiece Vocab's list, prefix and limit: one int32 array of list indices (or unk_id) per word.
        HOST ONLY, through the library's host implementation of the rule: a way to look at a split, not a hot path."""
        if not self.wordpiece:
            raise ValueError("split_words: not a WordPiece vocabulary")
        return split_words(self.words, words, self.unk_id, self._wp)

    # ---- host memory in and out ------------------------------------------------------------------------------------------------------------
    def _open_tokenizer(self):
        if not getattr(self._tokenizer, "_h", None):
            raise RuntimeError("the Vocab normalises and tokenizes on its Tokenizer, which has been closed")
        return self._tokenizer

    def encode_packed(self, utf8: np.ndarray, offsets: np.ndarray, out=None, _normalized: bool = False):
        """kgpu_encode_batch -> (ids[int32], id_offsets[uint64 n+1], status[uint8 n]): sentence i's sequence is
        ids[id_offsets[i]:id_offsets[i+1]].  out=(ids, id_offsets, status): caller-owned arrays to reuse (too small: KgpuError with
        KGPU_ERR_CAPACITY, nothing written)."""
        if self._normalize is not None and not _normalized:
            from .tokenizer import normalized_call

            return normalized_call(self._open_tokenizer(), self._normalize, self.encode_packed, utf8, offsets, out=out, _normalized=True)
        return batch_call(partial(_lib.lib().kgpu_encode_batch, self._h), utf8, offsets, np.int32, lambda total, n: total // 2 + n * (1 + self._extra) + 64,
                          ("ids[int32]", "id_offsets"), out=out)

    def encode_text(self, block):
        """kgpu_encode_text: a raw block of input (bytes or uint8 array) -> (ids, id_offsets, status) as encode_packed(*split_lines(block))
        gives them; the split and the trim run on the device."""
        if self._normalize is not None:
            from .tokenizer import normalized_call

            return normalized_call(self._open_tokenizer(), self._normalize, self.encode_packed, block=block, _normalized=True)

        def first(size):   # (as encode_packed sizes it, with every 16 bytes a possible line)
            lines = size // 16 + 1024
            return size // 2 + 64 + lines * self._extra, lines

        return block_call(partial(_lib.lib().kgpu_encode_text, self._h), block, np.int32, first)

    def encode(self, sentences: Sequence) -> List[np.ndarray]:
        """One int32 array per sentence (str or bytes)."""
        ids, ioff, _ = self.encode_packed(*pack_sentences(sentences))
        o = ioff.tolist()
        return [ids[o[i] : o[i + 1]] for i in range(len(o) - 1)]

    # ---- device memory out -----------------------------------------------------------------------------------------------------------------
    def encode_tensor(self, sentences: Sequence, width=None, pad_id: int = 0, normalize=None, return_spans: bool = False, split_sentences=False):
        """The sentences (str or bytes) as torch tensors on the device, in ONE DeviceContext batch: upload, tokenize, sync, encode, sync_lines.
        No id passes through host memory.  THE WHOLE BATCH MUST FIT DEVICE MEMORY (its text, 24 bytes per token and 4 bytes per id): cut a
        corpus into batches.  The batch is tokenized on a DeviceContext of this Vocab's Tokenizer, made by the first call: unlike the host
        forms, which work on a Vocab that has outlived its Words and its Tokenizer, encode_tensor NEEDS THE TOKENIZER OPEN (RuntimeError otherwise).
        width=None -> (ids int32 [total], offsets int64 [n + 1], status uint8 [n]); ids and offsets[:-1] are what torch.nn.EmbeddingBag takes.
        width=w    -> (ids int32 [n, w], lengths int64 [n] = min(L, w), status uint8 [n]); rows are cut after w elements (a cut row ends with
        eos_id when the vocabulary adds EOS) and filled with pad_id.
        normalize="NFC" / "NFKC" (None: the form the Vocab's Words handle was made with): the uploaded text is normalised on the device first
        (DeviceContext.normalize, sync_normalize) and the normalised buffers are what is tokenized and encoded: no text returns to the host.  The
        status is the tokenizer's, 4 where the normaliser left a line as it was and the tokenizer said 0.
        return_spans=True (kgpu_encode_device_spans) -> the tuple above and two more tensors, element for element beside ids: spans int32 [total, 4]
        ([n, w, 4] padded), the columns position, byte_len, start, end of the id's piece (a whole token where the header's rule 5 says so) inside its
        sentence -- columns 2:4 are character offsets, an offset_mapping -- and token_index int32 [total] ([n, w]), the index of the id's token among
        the sentence's records (EOS record and dropped tokens counted).  bos, eos and pad have zeros and -1.  With a normalisation form the text is
        normalised with its edit records (normalize_aligned) and the spans are in the coordinates of the SOURCE sentence, mapped on the device.
        split_sentences=True (or a _lib.sentence_opts(...) value): the entries are LINES -- paragraphs, documents -- and are cut into sentences on the
        device (DeviceContext.split_sentences; include/kanpyo_gpu.h, "sentences") behind the normalisation, which turns U+FF01 into '!' and U+FF62
        into U+300C first; the sentences are what is tokenized and encoded, no text returns to the host.  The tuple then has one row per SENTENCE
        and gains a last tensor, sentences int64 [S, 3]: line, byte_start, char_start of each in its (normalised) line.  Not with return_spans
        (ValueError): spans mapped through both the edits and the sentence starts are not offered."""
        import torch

        if width is not None and int(width) < 1:
            raise ValueError("width is 1 or more (None: ragged)")
        if split_sentences and return_spans:
            raise ValueError("split_sentences with return_spans is not offered: encode the sentences (Tokenizer.split_sentences) with return_spans instead")
        width = None if width is None else int(width)
        utf8, offs = pack_sentences(sentences)
        n, total = offs.size - 1, int(offs[-1])
        with self._ctx_lock:
            if self._ctx is None:
                if not getattr(self._tokenizer, "_h", None):
                    raise RuntimeError("encode_tensor tokenizes on a context of the Vocab's Tokenizer, which has been closed; encode_packed / encode_text still work")
                self._ctx = DeviceContext(self._tokenizer)
            ctx = self._ctx
            dev = torch.device("cuda", self._device)
            empty = partial(torch.empty, device=dev)
            d_utf8 = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
            form = self._normalize if normalize is None else _lib.normalize_form(normalize)
            d_nst = d_edits = d_eoff = None
            # 1. normalise: the normalised lines and their offsets take the input's place -- with the lines' edit records, a second capacity, for the spans' way back
            if form is not None:
                d_nst, d_noff = empty(max(n, 1), dtype=torch.uint8), empty(n + 1, dtype=torch.int64)
                d_eoff = empty(n + 1, dtype=torch.int64) if return_spans else None

                def norm_alloc(ncap, ecap=None):
                    return torch.zeros(ncap + 16, dtype=torch.uint8, device=dev), empty((ecap, 6), dtype=torch.int32) if return_spans else None

                def norm_enqueue(made, ncap, ecap=None):
                    if return_spans:
                        ctx.normalize_aligned(d_utf8.data_ptr(), d_off.data_ptr(), n, made[0].data_ptr(), ncap, d_noff.data_ptr(), d_nst.data_ptr(), made[1].data_ptr(), ecap,
                                              d_eoff.data_ptr(), form)
                    else:
                        ctx.normalize(d_utf8.data_ptr(), d_off.data_ptr(), n, made[0].data_ptr(), ncap, d_noff.data_ptr(), d_nst.data_ptr(), form)

                (total, *_), (d_utf8, d_edits) = _stage(dev, norm_alloc, norm_enqueue, ctx.try_sync_normalize_aligned if return_spans else ctx.try_sync_normalize,
                                                                  (total * 2 + 64, total // 8 + 64) if return_spans else (total * 2 + 64,))
                d_off = d_noff
            # 1b. sentences: the sentences and their offsets take the lines' place; a normaliser's status goes with the line to its sentences
            d_rec = None
            if split_sentences:
                sopts = split_sentences if isinstance(split_sentences, _lib.SentenceOpts) else None
                (n_sent, total), (d_utf8, d_soff, d_rec) = _stage(
                    dev, lambda cap: (torch.zeros(total + 16, dtype=torch.uint8, device=dev), empty(cap + 1, dtype=torch.int64), empty((max(cap, 1), 2), dtype=torch.int64)),
                    lambda made, cap: ctx.split_sentences(d_utf8.data_ptr(), d_off.data_ptr(), n, total, made[0].data_ptr(), made[1].data_ptr(), made[2].data_ptr(), cap, sopts),
                    ctx.try_sync_sentences, (2 * n + total // 32 + 64,))
                d_off, d_rec, n = d_soff[: n_sent + 1], d_rec[:n_sent], n_sent
                if d_nst is not None:
                    d_nst = d_nst[d_rec[:, 0]] if n else d_nst[:1]
            # 2. tokenize (a token buffer too small: once more with the count the device reports and 64, as tokenize_packed does)
            d_toff, d_st = empty(n + 1, dtype=torch.int64), empty(max(n, 1), dtype=torch.uint8)
            (n_tok,), d_tok = _stage(dev, lambda cap: empty((cap, 6), dtype=torch.int32),
                                     lambda d_tok, cap: ctx.tokenize(d_utf8.data_ptr(), d_off.data_ptr(), n, total, d_tok.data_ptr(), cap, d_toff.data_ptr(), d_st.data_ptr()),
                                     ctx.try_sync, (total // 2 + n + 64,), slack=64)
            # 3. encode.  Ragged, a plain Vocab: every record kept, and bos / eos: never too small; a WordPiece Vocab's tokens may give several ids each.
            # Padded: n x width is all there is
            d_ioff = empty(n + 1, dtype=torch.int64)

            def ids_alloc(id_cap):
                d_ids = empty(max(id_cap, 1), dtype=torch.int32) if width is None else empty((n, width), dtype=torch.int32)
                return (d_ids, empty(tuple(d_ids.shape) + (4,), dtype=torch.int32), torch.empty_like(d_ids)) if return_spans else (d_ids,)

            def ids_enqueue(made, id_cap):
                args = (self, d_utf8.data_ptr(), d_off.data_ptr(), n, d_tok.data_ptr(), d_toff.data_ptr(), made[0].data_ptr(), id_cap, d_ioff.data_ptr())
                if return_spans:
                    ctx.encode_spans(*args, made[1].data_ptr(), made[2].data_ptr(), d_edits.data_ptr() if d_edits is not None else 0,
                                     d_eoff.data_ptr() if d_eoff is not None else 0, width=width or 0, pad_id=int(pad_id))
                else:
                    ctx.encode(*args, width=width or 0, pad_id=int(pad_id))

            (count,), out = _stage(dev, ids_alloc, ids_enqueue, ctx.try_sync_lines, (n_tok + n * self._extra if width is None else n * width,), fixed=width is not None)
            if d_nst is not None:   # (on the device: the normaliser's 4 shows where the tokenizer said 0)
                d_st = torch.where((d_st == 0) & (d_nst == _lib.KGPU_SENT_NOT_NORMALIZED), d_nst, d_st)
        more = () if d_rec is None else (torch.stack([d_rec[:, 0], d_rec[:, 1] & 0xFFFFFFFF, (d_rec[:, 1] >> 32) & 0xFFFFFFFF], dim=1),)
        if width is None:
            return (out[0][:count], d_ioff, d_st[:n]) + tuple(t[:count] for t in out[1:]) + more
        return (out[0], torch.clamp(d_ioff[1:] - d_ioff[:-1], max=width), d_st[:n]) + out[1:] + more

    def encode_pairs_tensor(self, first: Sequence, second: Sequence = None, max_length: int = 512, stride: int = 0, truncation="only_second", windows: bool = True,
                            pad_id: int = 0, cls_id=None, sep_id=None, normalize=None, return_spans: bool = False) -> dict:
        """Model inputs on the device (include/kanpyo_gpu.h, "model inputs"): ONE encode_tensor batch over first + second (ragged; with spans when asked),
        then DeviceContext.pack over what it left in device memory -- rows `[cls] a [sep]` or `[cls] a [sep] b [sep]` of max_length slots, a sample that
        does not fit cut by `truncation` ("only_second", "only_first": the other side is kept whole; "longest_first") and, with windows=True, cut into
        overlapping windows that share `stride` elements, one row each.  No id passes through host memory.
        -> dict of tensors on the device: input_ids, token_type_ids, attention_mask (int32 [R, max_length]); row_offsets (int64 [n + 1]: sample i's rows
        are row_offsets[i] .. row_offsets[i + 1]); sample_of_row (int64 [R]: the overflow_to_sample_mapping of other libraries); status (uint8 [n]: 0
        whole, 1 cut, 2 no room -- zero rows); sentence_status (uint8, one per sentence of first + second: encode_tensor's); and with return_spans
        spans (int32 [R, max_length, 4]) and token_index (int32 [R, max_length]) as encode_tensor(return_spans=True) gives them, zeros and -1 on specials
        and pad.  With a normalisation form the spans are in SOURCE coordinates: the encode maps them, the pack only copies.
        cls_id / sep_id default to this Vocab's bos / eos ids (ValueError when it has none and none is given); a bos / eos the Vocab adds itself is trimmed
        from every sequence before it is packed.  second=None: singles ("only_second" is then "only_first": the one sequence is what is cut).
        windows=True with "longest_first" is not defined (the library refuses it): windows is taken as False there."""
        import torch

        from .pack import pack_opts

        pair = second is not None
        first = list(first)
        second = list(second) if pair else []
        if pair and len(second) != len(first):
            raise ValueError("first and second have the same number of entries")
        cls_id = self.bos_id if cls_id is None else cls_id
        sep_id = self.eos_id if sep_id is None else sep_id
        if cls_id is None or sep_id is None:
            raise ValueError("the Vocab adds no bos / eos of its own: give cls_id and sep_id")
        if truncation == "only_second" and not pair:
            truncation = "only_first"
        if truncation == "longest_first":
            windows = False
        opts = pack_opts(max_length, stride, truncation, windows, cls_id, sep_id, pad_id, trim_front=1 if self.bos_id is not None else 0,
                         trim_back=1 if self.eos_id is not None else 0)
        n = len(first)
        enc = self.encode_tensor(first + second, normalize=normalize, return_spans=return_spans)
        ids, ioff, sent_status = enc[0], enc[1], enc[2]
        n_ids = int(ids.numel())
        dev, ML = ids.device, int(max_length)
        d_roff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)

        def alloc(cap):
            rows = {k: torch.empty((cap, ML), dtype=torch.int32, device=dev) for k in ("input_ids", "token_type_ids", "attention_mask")}
            if return_spans:
                rows["spans"] = torch.empty((cap, ML, 4), dtype=torch.int32, device=dev)
                rows["token_index"] = torch.empty((cap, ML), dtype=torch.int32, device=dev)
            return rows

        def enqueue(rows, cap):
            self._ctx.pack(opts, n, ids.data_ptr(), ioff.data_ptr(), n_ids, rows["input_ids"].data_ptr(), cap, d_roff.data_ptr(), d_st.data_ptr(),
                           d_ids_b=ids.data_ptr() if pair else 0, d_off_b=ioff.data_ptr() + 8 * n if pair else 0,
                           d_type_ids=rows["token_type_ids"].data_ptr(), d_mask=rows["attention_mask"].data_ptr(),
                           d_spans_in=enc[3].data_ptr() if return_spans else 0, d_tix_in=enc[4].data_ptr() if return_spans else 0,
                           d_spans=rows["spans"].data_ptr() if return_spans else 0, d_tix=rows["token_index"].data_ptr() if return_spans else 0)

        with self._ctx_lock:   # (a row count beyond the guess: once more with the count the device reports)
            (R,), rows = _stage(dev, alloc, enqueue, self._ctx.try_sync_lines, (n + n_ids // max(1, ML - 3 - int(stride)) + 8,))
        out = {k: v[:R] for k, v in rows.items()}
        out["row_offsets"], out["status"], out["sentence_status"] = d_roff, d_st[:n], sent_status
        out["sample_of_row"] = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), d_roff[1:] - d_roff[:-1], output_size=R)
        return out

    def encode_spans(self, sentences: Sequence, normalize=None) -> List[tuple]:
        """The host-friendly form of encode_tensor(return_spans=True): per sentence (ids int32, spans[SPAN_DTYPE], token_index int32) as numpy arrays.
        The work is encode_tensor's, on the device; only the results are copied back."""
        ids, off, _, spans, tix = self.encode_tensor(sentences, normalize=normalize, return_spans=True)
        ids, tix, o = ids.cpu().numpy(), tix.cpu().numpy(), off.cpu().tolist()
        spans = np.ascontiguousarray(spans.cpu().numpy()).view(np.uint32).reshape(-1, 4).copy().view(SPAN_DTYPE).reshape(-1)
        return [(ids[o[i] : o[i + 1]], spans[o[i] : o[i + 1]], tix[o[i] : o[i + 1]]) for i in range(len(o) - 1)]

    # ---- the way back: text from ids (include/kanpyo_gpu.h, "text from ids") ---------------------------------------------------------------------
    def _decode_opts(self, separator, skip):
        from .decode import decode_opts

        if skip is None:   # the specials this handle puts around a sequence itself
            skip = [k for k in (self.bos_id, self.eos_id) if k is not None]
        return decode_opts(separator, skip)

    def decode_tensor(self, ids, offsets=None, separator=" ", skip=None):
        """Ids on the device (torch tensors, as encode_tensor leaves them) -> their text on the device, in ONE DeviceContext.decode: no id and no byte
        passes through host memory.  Ragged: ids int32 [total] with offsets int64 [n + 1]; padded: ids int32 [n, w] with offsets None (name the pad id in
        `skip`).  -> (text uint8 [bytes], text_offsets int64 [n + 1], status uint8 [n]): line s is text[text_offsets[s]:text_offsets[s + 1]], the words
        of its ids joined by `separator` (0..8 bytes), a WordPiece continuation joined to the word in front of it without its prefix; status 1: an id
        outside the list that `skip` does not name (it gives no text).  skip: at most 8 ids that give no text; None: this Vocab's bos and eos ids where
        set.  Like encode_tensor it runs on a context of the Vocab's Tokenizer, which has to be open."""
        import torch

        if offsets is None and ids.dim() != 2:
            raise ValueError("padded ids are [n, width]; ragged ids come with offsets")
        if ids.dtype != torch.int32 or (offsets is not None and offsets.dtype != torch.int64):
            raise ValueError("ids are int32, offsets int64")
        opts = self._decode_opts(separator, skip)
        ids = ids.contiguous()
        offsets = offsets.contiguous() if offsets is not None else None
        n = ids.shape[0] if offsets is None else offsets.numel() - 1
        width = ids.shape[1] if offsets is None else 0
        if n < 0 or (offsets is None and width < 1):
            raise ValueError("offsets needs n + 1 entries; a padded row has an id at least")
        with self._ctx_lock:
            if self._ctx is None:
                self._ctx = DeviceContext(self._open_tokenizer())
            ctx = self._ctx
            dev = torch.device("cuda", self._device)
            d_toff, d_st = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
            (count,), d_text = _stage(dev, lambda cap: torch.empty(max(cap, 1), dtype=torch.uint8, device=dev),
                                      lambda d_text, cap: ctx.decode(self, ids.data_ptr(), offsets.data_ptr() if offsets is not None else 0, n, d_text.data_ptr(), cap,
                                                                     d_toff.data_ptr(), d_st.data_ptr(), width=width, opts=opts),
                                      ctx.try_sync_lines, (ids.numel() * 8 + 64,))
        return d_text[:count], d_toff, d_st[:n]

    def decode(self, sequences: Sequence, separator=" ", skip=None) -> List[bytes]:
        """One line (bytes) per sequence of ids, over kgpu_decode_batch: host memory in and out, computed on the device.  separator and skip as
        decode_tensor takes them.  Works on a Vocab that has outlived its Words and its Tokenizer, as the host forms of encode do."""
        from .decode import host_call, lines

        seqs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in sequences]
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        if seqs:
            offs[1:] = np.cumsum([s.size for s in seqs])
        ids = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.int32)
        text, toff, _ = host_call(partial(_lib.lib().kgpu_decode_batch, self._h), ids, offs, 0, self._decode_opts(separator, skip))
        return lines(text, toff)

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
    def load(cls, words_handle, path, unk="<unk>", bos=None, eos=None, wordpiece=False, prefix="##", max_word_chars=100) -> "Vocab":
        """A Vocab over the file's list.  unk, bos, eos: WORDS that must be in the file (ValueError otherwise); bos / eos None: not added.
        wordpiece=True reads a BERT vocab.txt as it is: load(words, "vocab.txt", unk="[UNK]", bos="[CLS]", eos="[SEP]", wordpiece=True)."""
        return cls.from_words(words_handle, cls.read_words(path), unk, bos, eos, wordpiece, prefix, max_word_chars)

    @classmethod
    def from_words(cls, words_handle, words: Sequence, unk="<unk>", bos=None, eos=None, wordpiece=False, prefix="##", max_word_chars=100) -> "Vocab":
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
        return cls(words_handle, words, ids[0], ids[1], ids[2], wordpiece, prefix, max_word_chars)


def split_words_ends(vocab: Sequence, words: Sequence, unk_id: int, opts=None) -> List[tuple]:
    """kgpu_debug_wordpiece_split_ends: split_words with, per id, where its piece ends inside its word -> per word (ids int32 [k], ends uint32 [k, 2]:
    byte end, character end).  The one id of a word that gives unk_id ends where the word ends.  On the host, with no device and no handle."""
    vp, voff = pack_sentences([_word_bytes(w) for w in vocab])
    ip, ioff = pack_sentences([_word_bytes(w) for w in words])
    vp, ip = np.ascontiguousarray(vp), np.ascontiguousarray(ip)
    n = len(ioff) - 1
    ooff = np.zeros(n + 1, dtype=np.uint64)
    got = C.c_uint64(0)
    cap = int(ioff[-1]) + 1
    ids, ends = np.empty(cap, dtype=np.int32), np.zeros((cap, 2), dtype=np.uint32)
    _lib.check(_lib.lib().kgpu_debug_wordpiece_split_ends(ptr(vp), voff.ctypes.data, len(voff) - 1, C.byref(opts) if opts is not None else None, int(unk_id),
                                                          ptr(ip), ioff.ctypes.data, n, ids.ctypes.data, ends.ctypes.data, cap, ooff.ctypes.data, C.byref(got)))
    o = ooff.tolist()
    return [(ids[o[i] : o[i + 1]].copy(), ends[o[i] : o[i + 1]].copy()) for i in range(n)]


def split_words(vocab: Sequence, words: Sequence, unk_id: int, opts=None) -> List[np.ndarray]:
    """kgpu_debug_wordpiece_split: the WordPiece split of each of `words` by the list `vocab` (opts: wordpiece_opts(...), None: "##", 100), on the
    host, with no device and no handle -> one int32 array per word."""
    vp, voff = pack_sentences([_word_bytes(w) for w in vocab])
    ip, ioff = pack_sentences([_word_bytes(w) for w in words])
    vp, ip = np.ascontiguousarray(vp), np.ascontiguousarray(ip)
    n = len(ioff) - 1
    ooff = np.zeros(n + 1, dtype=np.uint64)
    got = C.c_uint64(0)
    cap = int(ioff[-1]) + 1   # (a piece is a byte at least; an over-long word is one id)
    ids = np.empty(cap, dtype=np.int32)
    _lib.check(_lib.lib().kgpu_debug_wordpiece_split(ptr(vp), voff.ctypes.data, len(voff) - 1, C.byref(opts) if opts is not None else None, int(unk_id),
                                                     ptr(ip), ioff.ctypes.data, n, ids.ctypes.data, cap, ooff.ctypes.data, C.byref(got)))
    o = ooff.tolist()
    return [ids[o[i] : o[i + 1]].copy() for i in range(n)]
