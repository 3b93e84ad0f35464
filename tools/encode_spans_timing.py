#!/usr/bin/env python
"""What a span and a token index per id cost beside the ids alone (python tools/encode_spans_timing.py [--parent-lib PATH] [rounds] [reps]): on
device-resident records, interleaved in one process, one context with one batch in flight -- the method of tools/align_timing.py.  Per corpus (the
40-character config, 16 384 sentences; a 4096-sentence batch of keyed, cfg 2 and cfg 3 sentences) and per vocabulary (plain; WordPiece, a BERT-like list):
  (1) kgpu_encode_device of the library at PATH: the parent commit's build (only with --parent-lib; its own dictionary, vocabulary and context)
  (2) kgpu_encode_device of this tree: the same kernels, so it must sit within the spread of (1)
  (3) kgpu_encode_device_spans without edits, on the same records
  (d) kgpu_encode_device and (4) kgpu_encode_device_spans WITH edits, on the records of the same text with 10 % of its characters half-width or
      full-width, normalised with its edit records and tokenized once, outside the timing: (4)/(d) is the cost on equal input, (4)/(1) what the issue asks
Every repetition is `rounds` interleaved rounds; its medians are printed, and at the end the spread of the medians over the repetitions."""
import contextlib, ctypes as C, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from kanpyo_amd import Tokenizer, _lib, normalize_host, synth
from kanpyo_amd.device import DeviceContext
from kanpyo_amd.tokenizer import pack_sentences
argv = sys.argv[1:]
parent_path = argv.pop(argv.index("--parent-lib") + 1) if "--parent-lib" in argv else None
if parent_path: argv.remove("--parent-lib")
rounds = int(argv[0]) if len(argv) > 0 else 15
reps = int(argv[1]) if len(argv) > 1 else 5
HALF = "ｱｲｳｴｵｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾅﾆﾇﾈﾉ"
FULL = "ＡＢＣＤＥＦＧＨＩＪ０１２３４５６７８９"
SPECIALS = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"]
def dirty(s, rng):   # every tenth character, on average, becomes a half-width kana or a full-width letter or digit
    pool = HALF + FULL
    return "".join(pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.1 else c for c in s)
MAIN = _lib.lib()
PARENT = None
if parent_path:   # a second library in this process, with the signatures of the symbols it shares with this tree's
    PARENT = C.CDLL(os.path.abspath(parent_path))
    for name, f in list(vars(MAIN).items()):
        if isinstance(f, C._CFuncPtr) and hasattr(PARENT, name):
            g = getattr(PARENT, name); g.argtypes, g.restype = f.argtypes, f.restype
@contextlib.contextmanager
def using(L):   # the binding reaches its library through _lib.lib(): handles made under `using(PARENT)` are the parent library's, and so are their calls
    saved, _lib._lib = _lib._lib, L
    try: yield
    finally: _lib._lib = saved
sd = synth.build_dict(); known, unk = synth.feature_tables(sd); keys = synth.record_surfaces(sd)
dev = torch.device("cuda", 0)
class Side:   # a dictionary handle, its Words handle and a context of one library
    def __init__(self, L):
        self.L = L
        with using(L):
            self.tok = Tokenizer(sd.dict); self.tok.set_features(known, unk); self.words = self.tok.words(); self.ctx = DeviceContext(self.tok)
    def vocab(self, words, wordpiece):
        with using(self.L): return self.words.vocabulary(words, 1, 2, 3, wordpiece=wordpiece)
main = Side(MAIN); parent = Side(PARENT) if PARENT else None
def corpora():
    rng = random.Random(7); longer = [k for k in keys if len(k) >= 2]
    keyed = ["".join(rng.choice(longer) for _ in range(rng.randrange(1, 12))) for _ in range(2800)]
    yield "cfg2 x 16384", synth.make_corpus(sd, 16384, 1, "cfg2")
    yield "mixed x 4096", keyed + synth.make_corpus(sd, 1100, 7, "cfg2") + synth.make_corpus(sd, 196, 8, "cfg3")
class Batch:   # a corpus normalised with its edit records and tokenized on the device, once: text, offsets, records, record offsets, edits, edit offsets
    def __init__(self, sents):
        utf8, offs = pack_sentences(sents); n, total = len(sents), int(offs[-1]); ctx = main.ctx
        d_u = torch.from_numpy(np.concatenate([utf8, np.zeros(16, dtype=np.uint8)])).to(dev); d_o = torch.from_numpy(offs.astype(np.int64)).to(dev)
        cap = 3 * total + 64
        self.text = torch.zeros(cap + 16, dtype=torch.uint8, device=dev); self.off = torch.empty(n + 1, dtype=torch.int64, device=dev); st = torch.empty(n, dtype=torch.uint8, device=dev)
        self.edits = torch.zeros(total * 24 + 24, dtype=torch.uint8, device=dev); self.eoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.normalize_aligned(d_u.data_ptr(), d_o.data_ptr(), n, self.text.data_ptr(), cap, self.off.data_ptr(), st.data_ptr(), self.edits.data_ptr(), total, self.eoff.data_ptr(), "NFKC")
        nbytes, self.n_edits = ctx.sync_normalize_aligned()
        tcap = nbytes + n + 64
        self.tok = torch.empty((tcap, 6), dtype=torch.int32, device=dev); self.toff = torch.empty(n + 1, dtype=torch.int64, device=dev); kst = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.tokenize(self.text.data_ptr(), self.off.data_ptr(), n, nbytes, self.tok.data_ptr(), tcap, self.toff.data_ptr(), kst.data_ptr()); self.n_tok = ctx.sync()
        self.n, self.cap = n, 4 * nbytes + 2 * n + 64   # (a piece is a byte at least)
        self.ids = torch.empty(self.cap, dtype=torch.int32, device=dev); self.ioff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.spans = torch.empty((self.cap, 4), dtype=torch.int32, device=dev); self.tix = torch.empty(self.cap, dtype=torch.int32, device=dev)
    def encode(self, side, v):
        with using(side.L):
            side.ctx.encode(v, self.text.data_ptr(), self.off.data_ptr(), self.n, self.tok.data_ptr(), self.toff.data_ptr(), self.ids.data_ptr(), self.cap, self.ioff.data_ptr())
            return side.ctx.sync_lines()
    def spans_call(self, v, edits):
        main.ctx.encode_spans(v, self.text.data_ptr(), self.off.data_ptr(), self.n, self.tok.data_ptr(), self.toff.data_ptr(), self.ids.data_ptr(), self.cap, self.ioff.data_ptr(),
                              self.spans.data_ptr(), self.tix.data_ptr(), self.edits.data_ptr() if edits else 0, self.eoff.data_ptr() if edits else 0)
        return main.ctx.sync_lines()
def chars_of(w):   # a character starts at byte 0 and at every byte that is not 10xxxxxx
    st = [i for i in range(len(w)) if i == 0 or w[i] & 0xC0 != 0x80]
    return [w[a:b] for a, b in zip(st, st[1:] + [len(w)])]
def lists(sents):   # a plain list of the 4000 most frequent words; a BERT-like list: 500 words, then every character c of the words and ##c
    counts = main.words.counter(); counts.add_packed(*pack_sentences(sents)); order = [w for w, _ in counts.most_common()]; counts.close()
    chars = sorted({c for w in order for c in chars_of(w)})
    head = [w for w in order[:500] if w not in SPECIALS]
    return SPECIALS + [w for w in order[:4000] if w not in SPECIALS], SPECIALS + head + [c for c in chars if c not in set(head) and c not in SPECIALS] + [b"##" + c for c in chars]
print(f"{reps} repetitions of {rounds} interleaved rounds, one context with one batch in flight; medians in us" + ("" if parent else "; NO --parent-lib: arm (1) is not run"))
for name, sents in corpora():
    clean = [normalize_host(x).decode() for x in sents]; rng = np.random.default_rng(5)
    bc, bd = Batch(clean), Batch([dirty(s, rng) for s in clean])
    assert bc.n_edits == 0 and bd.n_edits > 0
    for kind, words in zip(("plain", "wordpiece"), lists(clean)):
        v = main.vocab(words, kind == "wordpiece"); pv = parent.vocab(words, kind == "wordpiece") if parent else None
        arms = {"2": lambda: bc.encode(main, v), "3": lambda: bc.spans_call(v, False), "d": lambda: bd.encode(main, v), "4": lambda: bd.spans_call(v, True)}
        if parent: arms = {"1": lambda: bc.encode(parent, pv), **arms}
        for f in arms.values():   # warm-up: code objects loaded, scratch sized, clocks up
            for _ in range(3): f()
        n_ids, n_ids_d = arms["2"](), arms["d"]()
        assert arms["3"]() == n_ids and arms["4"]() == n_ids_d and (not parent or arms["1"]() == n_ids), "every arm of one input gives the same number of ids"
        print(f"{name}, {kind} ({len(words)} entries): {bc.n_tok} records -> {n_ids} ids; 10 % half-/full-width: {bd.n_tok} records, {bd.n_edits} edits -> {n_ids_d} ids")
        meds = {k: [] for k in arms}
        for r in range(reps):
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, f in arms.items():
                    torch.cuda.synchronize(); t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
            for k in arms: meds[k].append(float(np.median(times[k])) * 1e6)
            print(f"  rep {r}: " + "  ".join(f"({k}) {meds[k][-1]:.1f}" for k in arms))
        for k in arms:
            a = np.array(meds[k]); print(f"  ({k}) median of medians {np.median(a):.1f} us, min {a.min():.1f}, max {a.max():.1f}, spread {(a.max() - a.min()) / np.median(a) * 100:.1f} %")
        base = "1" if parent else "2"
        ratio = lambda x, y: np.array(meds[x]) / np.array(meds[y])   # noqa: E731
        for x, y in (("2", "1"), ("3", base), ("4", base), ("4", "d")):
            if y in meds and x != y:
                q = ratio(x, y); print(f"  ({x})/({y}): median {np.median(q):.3f} (min {q.min():.3f}, max {q.max():.3f})")
        v.close()
        if pv is not None:
            with using(PARENT): pv.close()
sys.stdout.flush()
os._exit(0)   # (the handles of two libraries: no destructor runs against the wrong one)
