#!/usr/bin/env python
"""What the sentence split costs and what it buys (python tools/sentence_rate.py [sentences] [per_doc] [rounds] [encode_sentences] [--out FILE]), on device-resident
input, interleaved in one process and one build:
  split   GB/s of kgpu_split_sentences_device beside kgpu_split_lines_device over the same text -- `sentences` cfg2 sentences of the synthetic corpus
          with a U+3002 appended, once one per line and once `per_doc` per line ("documents"); the line split reads the lines joined by '\\n'.
          Both move about the same bytes per input byte; the sentence split adds the offsets, two more scans and a third pass over the text.
  encode  sentences/s and Gchar/s of Vocab.encode_tensor over the documents, split_sentences=True beside whole lines: what tells a user whether to
          split (`encode_sentences` of them, 12800 unless given: one batch).  The two tokenize differently at the boundaries (BOS / EOS instead of a connection): this compares speed, not output.
One context, one batch in flight.  Three repetitions of `rounds` interleaved rounds each: the median of each repetition is printed, and their spread.

Each leg run by tools/measure.py, a process of its own under a time limit."""
import measure


def _corpora(sd, n, per_doc):
    from kanpyo_amd import synth

    sents = [s + "。" for s in synth.make_corpus(sd, n, 1, "cfg2")]
    docs = ["".join(sents[i : i + per_doc]) for i in range(0, n, per_doc)]
    return sents, docs


def split_leg(say, n, per_doc, rounds):
    import numpy as np
    import torch

    from kanpyo_amd import split_sentences_host
    from kanpyo_amd.device import DeviceContext
    from kanpyo_amd.tokenizer import pack_sentences, split_lines

    sd, tok, _, _ = measure.synthetic_tokenizer()
    dev = torch.device("cuda", 0)
    ctx = DeviceContext(tok)
    say(f"{n} cfg2 sentences + U+3002; documents of {per_doc}; 3 repetitions of {rounds} interleaved rounds, one batch in flight")
    for name, lines in zip(("one sentence per line", f"{per_doc} sentences per line"), _corpora(sd, n, per_doc)):
        utf8, offs = pack_sentences(lines)
        total, nl = int(utf8.size), len(lines)
        d_text = torch.from_numpy(np.concatenate([utf8, np.zeros(16, np.uint8)])).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        block = np.frombuffer("".join(x + "\n" for x in lines).encode(), dtype=np.uint8)
        d_block = torch.from_numpy(block.copy()).to(dev)
        cap = total // 3 + nl + 64
        d_out, d_ooff, d_rec = torch.empty(block.size + 64, dtype=torch.uint8, device=dev), torch.empty(cap + 1, dtype=torch.int64, device=dev), torch.empty((cap, 2), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)

        def sentences():
            ctx.split_sentences(d_text.data_ptr(), d_off.data_ptr(), nl, total, d_out.data_ptr(), d_ooff.data_ptr(), d_rec.data_ptr(), cap)
            return ctx.sync_sentences()

        def newlines():
            ctx.split_lines(d_block.data_ptr(), int(block.size), d_out.data_ptr(), d_ooff.data_ptr(), cap + 1)
            return ctx.sync_split()

        arms = {"sentences": sentences, "lines": newlines}
        for f in arms.values():
            for _ in range(3):
                f()
        want = len(split_sentences_host(utf8, offs)[2])   # (the corpus has terminators and brackets of its own)
        assert sentences()[0] == want and newlines()[0] == len(split_lines(block)[1]) - 1
        meds = measure.interleaved(arms, 3, rounds, before=torch.cuda.synchronize)
        s, l = measure.summary(meds["sentences"]), measure.summary(meds["lines"])
        say(f"{name}: {nl} lines, {total} bytes, {want} sentences")
        say(f"  sentence split: {[round(t * 1e6) for t in meds['sentences']]} us; median {s[0] * 1e6:.0f} us (spread {s[1] * 100:.0f} %) = {total / s[0] / 1e9:.1f} GB/s")
        say(f"  line split:     {[round(t * 1e6) for t in meds['lines']]} us; median {l[0] * 1e6:.0f} us (spread {l[1] * 100:.0f} %) = {block.size / l[0] / 1e9:.1f} GB/s")
        say(f"  per byte, sentence split / line split = {(s[0] / total) / (l[0] / block.size):.2f}")
    return True


def encode_leg(say, n, per_doc, rounds):
    import torch

    from kanpyo_amd.tokenizer import pack_sentences

    sd, tok, _, _ = measure.synthetic_tokenizer()
    sents, docs = _corpora(sd, n, per_doc)
    toks, toff, _ = tok.tokenize_packed(*pack_sentences(sents[:2000]))
    surfaces = {s.encode()[int(t["position"]) : int(t["position"]) + int(t["byte_len"])] for i, s in enumerate(sents[:2000]) for t in toks[int(toff[i]) : int(toff[i + 1])] if int(t["byte_len"])}
    v = tok.words().vocabulary([b"<unk>", b"<s>", b"</s>"] + sorted(surfaces), 0, 1, 2)
    chars = sum(len(d) for d in docs)
    arms = {"split": lambda: v.encode_tensor(docs, split_sentences=True), "whole": lambda: v.encode_tensor(docs)}
    for f in arms.values():
        for _ in range(2):
            f()
    from kanpyo_amd import split_sentences_host

    rows = int(arms["split"]()[1].numel()) - 1
    assert rows == len(split_sentences_host(*pack_sentences(docs))[2]), rows
    meds = measure.interleaved(arms, 3, rounds, before=torch.cuda.synchronize)
    say(f"encode_tensor over {len(docs)} documents of {per_doc} sentences ({rows} sentences, {chars} characters, upload included); 3 repetitions of {rounds} rounds")
    for k, what in (("split", "split_sentences=True"), ("whole", "whole lines         ")):
        m, spread = measure.summary(meds[k])
        say(f"  {what}: {[round(t * 1e3, 2) for t in meds[k]]} ms; median {m * 1e3:.2f} ms (spread {spread * 100:.0f} %) = {rows / m / 1e6:.2f} M sentences/s, {chars / m / 1e9:.3f} Gchar/s")
    say(f"  whole lines / split = {measure.summary(meds['whole'])[0] / measure.summary(meds['split'])[0]:.2f}")
    return True


if __name__ == "__main__":
    ap = measure.parser(__doc__)
    ap.add_argument("sentences", nargs="?", type=int, default=65536)
    ap.add_argument("per_doc", nargs="?", type=int, default=50)
    ap.add_argument("rounds", nargs="?", type=int, default=9)
    ap.add_argument("encode_sentences", nargs="?", type=int, default=12800)
    args = ap.parse_args()
    n = args.sentences - args.sentences % args.per_doc
    measure.main(__file__, args, {"split": (lambda say: split_leg(say, n, args.per_doc, args.rounds), 400),
                                  "encode": (lambda say: encode_leg(say, args.encode_sentences - args.encode_sentences % args.per_doc, args.per_doc, args.rounds), 500)},
                 leg_args=[str(args.sentences), str(args.per_doc), str(args.rounds), str(args.encode_sentences)], header=lambda: f"# tools/sentence_rate.py, library {measure.library_hash()}")
