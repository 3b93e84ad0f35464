#!/usr/bin/env python
"""What a span and a token index per id cost beside the ids alone (python tools/encode_spans_timing.py [--parent-lib PATH] [rounds] [reps]): on
device-resident records, interleaved in one process, one context with one batch in flight -- the method of tools/align_timing.py.  Per corpus (the
40-character config, 16 384 sentences; a 4096-sentence batch of keyed, cfg 2 and cfg 3 sentences) and per vocabulary (plain; WordPiece, a BERT-like list):
  (1) kgpu_encode_device of the library at PATH: the parent commit's build (only with --parent-lib; its own dictionary, vocabulary and context)
  (2) kgpu_encode_device of this tree: the same kernels, so it must sit within the spread of (1)
  (3) kgpu_encode_device_spans without edits, on the same records
  (d) kgpu_encode_device and (4) kgpu_encode_device_spans WITH edits, on the records of the same text with 10 % of its characters half-width or
      full-width, normalised with its edit records and tokenized once, outside the timing: (4)/(d) is the cost on equal input, (4)/(1) what the issue asks
Every repetition is `rounds` interleaved rounds; its medians are printed, and at the end the spread of the medians over the repetitions.

One leg run by tools/measure.py, a process of its own under a time limit -- both libraries of --parent-lib live in it --; the repetitions are
measure.interleaved() with a device synchronize ahead of each call."""
import os
import sys

import measure

SPECIALS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"]


def chars_of(w):   # a character starts at byte 0 and at every byte that is not 10xxxxxx
    st = [i for i in range(len(w)) if i == 0 or w[i] & 0xC0 != 0x80]
    return [w[a:b] for a, b in zip(st, st[1:] + [len(w)])]


def leg(say, parent_path, rounds, reps):
    import contextlib
    import ctypes as C
    import random

    import numpy as np
    import torch

    from kanpyo_amd import Tokenizer, _lib, normalize_host, synth
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences

    MAIN = _lib.lib()
    PARENT = None
    if parent_path:   # a second library in this process, with the signatures of the symbols it shares with this tree's
        PARENT = C.CDLL(os.path.abspath(parent_path))
        for name, f in list(vars(MAIN).items()):
            if isinstance(f, C._CFuncPtr) and hasattr(PARENT, name):
                g = getattr(PARENT, name)
                g.argtypes, g.restype = f.argtypes, f.restype

    @contextlib.contextmanager
    def using(L):   # the binding reaches its library through _lib.lib(): handles made under `using(PARENT)` are the parent library's, and so are their calls
        saved, _lib._lib = _lib._lib, L
        try:
            yield
        finally:
            _lib._lib = saved

    sd = synth.build_dict()
    known, unk = synth.feature_tables(sd)
    keys = synth.record_surfaces(sd)
    dev = torch.device("cuda", 0)

    class Side:   # a dictionary handle, its Words handle and a context of one library
        def __init__(self, L):
            self.L = L
            with using(L):
                self.tok = Tokenizer(sd.dict)
                self.tok.set_features(known, unk)
                self.words = self.tok.words()
                self.ctx = DeviceContext(self.tok)

        def vocab(self, words, wordpiece):
            with using(self.L):
                return self.words.vocabulary(words, 1, 2, 3, wordpiece=wordpiece)

    main = Side(MAIN)
    parent = Side(PARENT) if PARENT else None

    def corpora():
        rng = random.Random(7)
        longer = [k for k in keys if len(k) >= 2]
        keyed = ["".join(rng.choice(longer) for _ in range(rng.randrange(1, 12))) for _ in range(2800)]
        yield "cfg2 x 16384", synth.make_corpus(sd, 16384, 1, "cfg2")
        yield "mixed x 4096", keyed + synth.make_corpus(sd, 1100, 7, "cfg2") + synth.make_corpus(sd, 196, 8, "cfg3")

    class Batch:   # a corpus normalised with its edit records and tokenized on the device, once: text, offsets, records, record offsets, edits, edit offsets
        def __init__(self, sents):
            utf8, offs = pack_sentences(sents)
            n, total, ctx = len(sents), int(offs[-1]), main.ctx
            d_u = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_o = torch.from_numpy(offs.astype(np.int64)).to(dev)
            cap = 3 * total + 64
            self.text, self.off, st = torch.zeros(cap + 16, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            self.edits, self.eoff = torch.zeros(total * 24 + 24, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ctx.normalize_aligned(d_u.data_ptr(), d_o.data_ptr(), n, self.text.data_ptr(), cap, self.off.data_ptr(), st.data_ptr(), self.edits.data_ptr(), total, self.eoff.data_ptr(), "NFKC")
            nbytes, self.n_edits = ctx.sync_normalize_aligned()
            tcap = nbytes + n + 64
            self.tok, self.toff, kst = torch.empty((tcap, 6), dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            ctx.tokenize(self.text.data_ptr(), self.off.data_ptr(), n, nbytes, self.tok.data_ptr(), tcap, self.toff.data_ptr(), kst.data_ptr())
            self.n_tok = ctx.sync()
            self.n, self.cap = n, 4 * nbytes + 2 * n + 64   # (a piece is a byte at least)
            self.ids, self.ioff = torch.empty(self.cap, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
            self.spans, self.tix = torch.empty((self.cap, 4), dtype=torch.int32, device=dev), torch.empty(self.cap, dtype=torch.int32, device=dev)

        def encode(self, side, v):
            with using(side.L):
                side.ctx.encode(v, self.text.data_ptr(), self.off.data_ptr(), self.n, self.tok.data_ptr(), self.toff.data_ptr(), self.ids.data_ptr(), self.cap, self.ioff.data_ptr())
                return side.ctx.sync_lines()

        def spans_call(self, v, edits):
            main.ctx.encode_spans(v, self.text.data_ptr(), self.off.data_ptr(), self.n, self.tok.data_ptr(), self.toff.data_ptr(), self.ids.data_ptr(), self.cap, self.ioff.data_ptr(),
                                  self.spans.data_ptr(), self.tix.data_ptr(), self.edits.data_ptr() if edits else 0, self.eoff.data_ptr() if edits else 0)
            return main.ctx.sync_lines()

    def lists(sents):   # a plain list of the 4000 most frequent words; a BERT-like list: 500 words, then every character c of the words and ##c
        counts = main.words.counter()
        counts.add_packed(*pack_sentences(sents))
        order = [w for w, _ in counts.most_common()]
        counts.close()
        chars = sorted({c for w in order for c in chars_of(w)})
        head = [w for w in order[:500] if w not in SPECIALS]
        return SPECIALS + [w for w in order[:4000] if w not in SPECIALS], SPECIALS + head + [c for c in chars if c not in set(head) and c not in SPECIALS] + [b"##" + c for c in chars]

    say(f"{reps} repetitions of {rounds} interleaved rounds, one context with one batch in flight; medians in us" + ("" if parent else "; NO --parent-lib: arm (1) is not run"))
    for name, sents in corpora():
        clean = [normalize_host(x).decode() for x in sents]
        rng = np.random.default_rng(5)
        bc, bd = Batch(clean), Batch([measure.dirty(s, rng) for s in clean])
        assert bc.n_edits == 0 and bd.n_edits > 0
        for kind, words in zip(("plain", "wordpiece"), lists(clean)):
            v = main.vocab(words, kind == "wordpiece")
            pv = parent.vocab(words, kind == "wordpiece") if parent else None
            arms = {"2": lambda: bc.encode(main, v), "3": lambda: bc.spans_call(v, False), "d": lambda: bd.encode(main, v), "4": lambda: bd.spans_call(v, True)}
            if parent:
                arms = {"1": lambda: bc.encode(parent, pv), **arms}
            for f in arms.values():   # warm-up: code objects loaded, scratch sized, clocks up
                for _ in range(3):
                    f()
            n_ids, n_ids_d = arms["2"](), arms["d"]()
            assert arms["3"]() == n_ids and arms["4"]() == n_ids_d and (not parent or arms["1"]() == n_ids), "every arm of one input gives the same number of ids"
            say(f"{name}, {kind} ({len(words)} entries): {bc.n_tok} records -> {n_ids} ids; 10 % half-/full-width: {bd.n_tok} records, {bd.n_edits} edits -> {n_ids_d} ids")
            meds = {k: [x * 1e6 for x in m] for k, m in measure.interleaved(arms, reps, rounds, before=torch.cuda.synchronize).items()}
            for r in range(reps):
                say(f"  rep {r}: " + "  ".join(f"({k}) {meds[k][r]:.1f}" for k in arms))
            for k in arms:
                a = meds[k]
                say(f"  ({k}) median of medians {measure.summary(a)[0]:.1f} us, min {min(a):.1f}, max {max(a):.1f}, spread {measure.summary(a)[1] * 100:.1f} %")
            base = "1" if parent else "2"
            for x, y in (("2", "1"), ("3", base), ("4", base), ("4", "d")):
                if y in meds and x != y:
                    q = [p / r for p, r in zip(meds[x], meds[y])]
                    say(f"  ({x})/({y}): median {measure.summary(q)[0]:.3f} (min {min(q):.3f}, max {max(q):.3f})")
            v.close()
            if pv is not None:
                with using(PARENT):
                    pv.close()
    sys.stdout.flush()
    os._exit(0)   # (the handles of two libraries: no destructor runs against the wrong one)


if __name__ == "__main__":
    ap = measure.parser(__doc__)
    ap.add_argument("--parent-lib", default=None, metavar="PATH")
    ap.add_argument("rounds", nargs="?", type=int, default=15)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    measure.main(__file__, args, {"measure": (lambda say: leg(say, args.parent_lib, args.rounds, args.reps), 500)},
                 leg_args=[*(["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else []), str(args.rounds), str(args.reps)])
