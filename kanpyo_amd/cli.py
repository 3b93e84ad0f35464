"""`python -m kanpyo_amd tokenize [-c DICT] [INPUT]`: the reference's `kanpyo tokenize` (src/bin/kanpyo.rs:106-126, 174-197) on the device.

Its stdout is the reference binary's, byte for byte: one `surface\\tf1,f2,...` line per token, sentences one after the other.  With INPUT
that one string is tokenized untrimmed; without it stdin is read line by line (split at '\\n', trailing Unicode White_Space trimmed, as
read_line + trim_end do) -- here in blocks of whole lines, each tokenized and rendered on the device in one kgpu_tokenize_batch_lines
call and written out as soon as it is done.  `--split device` hands each block to kgpu_tokenize_text_lines as it was read: the split and the
trim run on the device too (`--split host`, the default, splits with kgpu_split_lines on the host).  A line that is not UTF-8 ends the
run as the reference's `expect` panic does: the lines before it are printed, exit status 101.  No subcommand means `tokenize` from stdin.
`--nbest K` (1..64; NOT an option of the reference: what `mecab -N K` prints) prints for every input line its K lowest-cost paths, best first (fewer where
the lattice has fewer, none where EOS is unreachable): each path is the lines of its tokens, ending with its EOS line, exactly as `tokenize` prints
one.  The paths are found on the device (kgpu_tokenize_batch_nbest); their lines are rendered on the host from the records -- which needs the lines
there: `--split device` with it is an argument error.
`--marginal [--all-morphs] [--min-prob P] [--theta T]` and `--sample N [--seed S] [--theta T]` (NOT options of the reference either: `mecab -m` / `-a`
and `mecab -l --theta`) read the lattice as a distribution, P(path) proportional to exp(-T cost): --marginal prints `tokenize`'s lines with `\t%.6f`,
the token's marginal probability, appended (--all-morphs: a line for every node whose marginal is at least P); --sample N prints N tokenizations drawn
from the lattice, one after the other as --nbest prints its paths.  Computed on the device (kgpu_tokenize_batch_marginals / _samples), rendered on the
host: not with `--split device`, not with --nbest.
`--mode {normal,search,extended} [--mode-penalties KL,KP,OL,OP]` (NOT an option of the reference: what Kuromoji and Kagome offer for search indexing)
prints every line's best path under a length penalty on long words, so that a compound gives way to the parts the dictionary has; extended also cuts
unknown words into characters; normal prints what `tokenize` prints.  Decoded on the device (kgpu_tokenize_batch_mode), rendered on the host: not with
`--split device`, --nbest, --marginal or --sample.

`python -m kanpyo_amd graphviz [INPUT] [-c DICT] [-f/--full-state] [--dpi N]`: the reference's `kanpyo graphviz` (src/bin/kanpyo.rs:31-48,
127-148 over src/graphviz.rs:30-163): the lattice of ONE sentence as a DOT document, built and rendered on the device in one
kgpu_graphviz_batch call.  With INPUT that string is drawn untrimmed; without it ONE line of stdin is read and trimmed (read_line +
trim_end, not a loop: further lines are ignored, empty stdin is the empty sentence).  A first line that is not UTF-8 ends with status 101.

`python -m kanpyo_amd wakati [INPUT] [-c DICT] [--field N | --base-form | --reading | --pronunciation] [--drop POS[,POS...] | --keep POS[,POS...]]
[--separator S] [--split host|device]`: NOT a subcommand of the reference -- wakati-gaki, what `mecab -Owakati` prints: every input line
becomes one output line, its words separated by S (one byte, default a space), rendered on the device (kgpu_tokenize_batch_words /
kgpu_tokenize_text_words).  --field N prints feature N of each token's row instead of the surface (--base-form, --reading, --pronunciation:
6, 7, 8, IPADIC's columns; the surface where a row has no such feature, or it is empty or "*"); --drop / --keep filter tokens by feature 0,
the part of speech.  stdin is handled as `tokenize` handles it: blocks of whole lines, and a line that is not UTF-8 ends the run with status
101 after the lines before it.

`python -m kanpyo_amd count [INPUT] [-c DICT] [--field N | --base-form | --reading | --pronunciation] [--drop POS[,POS...] | --keep POS[,POS...]]
[--top N] [--split host|device] [--skip-invalid]`: NOT a subcommand of the reference either -- the word frequencies of the whole input, what
`wakati | tr ' ' '\n' | sort | uniq -c | sort -rn` gives, accumulated on the device (kgpu_count_batch / kgpu_count_text) and printed at the end
as `count\tword` lines, by count descending and then by the word's bytes ascending; --top N prints the first N.  The words and the filter are
wakati's.  A line that is not UTF-8 ends the run with status 101, its 1-based line number on stderr and NOTHING on stdout -- a partial
frequency table is worse than none; with --skip-invalid such lines are skipped, their numbers go to stderr and the status is 0.

`python -m kanpyo_amd encode [INPUT] -c DICT --vocab FILE [--wordpiece [--prefix S] [--max-word-chars N]] [--field N | --base-form | --reading | --pronunciation] [--drop POS[,POS...] | --keep POS[,POS...]]
[--unk WORD] [--bos WORD] [--eos WORD] [--offsets] [--max-length N [--stride S] [--truncation T] [--pair]] [--split host|device] [--skip-invalid]`: NOT a subcommand of the reference either -- every input line becomes
one output line, the vocabulary ids of its words in decimal, separated by one space (kgpu_encode_batch / kgpu_encode_text; the decimal text is made
on the host).  FILE has one word per line, line k (0-based) is id k: `count ... | cut -f2` makes one.  --unk (default "<unk>"), --bos and --eos name
words that must be in the file (exit status 2 otherwise); a word outside the file gets --unk's id, --bos / --eos put theirs around every line's ids.
The words and the filter are wakati's.  A line that is not UTF-8 is handled as `count` handles it: status 101, its line number on stderr and NOTHING
on stdout; with --skip-invalid such a line prints its bos / eos only.  --offsets (include/kanpyo_gpu.h, "ids with spans") is an inspection tool: one
output line PER ID, `id\tstart\tend\ttoken_index\ttext`, and `EOS` behind each input line -- start and end are character positions in the line as it was
given (through --normalize's edit records), text is those characters, token_index the id's token among the line's records; bos and eos print
`id\t0\t0\t-1\t`.  Ids, spans and indices are made on the device (Vocab.encode_tensor(return_spans=True)), the text is formatted on the host -- which needs
the lines there: stdin's blocks are split on the host whatever --split says.  --max-length N (include/kanpyo_gpu.h, "model inputs") prints MODEL INPUT
ROWS instead: one output line per row, `sample\tids...` up to the pad, sample the 0-based number of the input line the row belongs to -- a line that does not
fit N ids with its specials is cut by --truncation (only_second, the default, only_first, longest_first) and, but for longest_first, cut into windows that
share --stride ids (default 0).  With --pair an input line is `a<TAB>b` (a line without a tab has an empty b).  The rows are made on the device
(Vocab.encode_pairs_tensor); the specials are --bos and --eos, which this form needs; stdin's blocks are split on the host.

`python -m kanpyo_amd decode [INPUT] -c DICT --vocab FILE [--wordpiece [--prefix S]] [--separator S] [--skip ID[,ID...]]`: NOT a subcommand of the
reference either -- the way back from `encode` (include/kanpyo_gpu.h, "text from ids"): every input line is decimal ids separated by spaces, what
`encode` prints, and becomes one output line, the words of its ids joined by --separator (0 to 8 bytes, default a space; '' is allowed here), on the
device (kgpu_decode_batch).  With --wordpiece a continuation piece joins the word in front of it without its prefix.  --skip names at most 8 ids that
give no text (a bos, an eos, a pad); an id outside FILE gives none either.  `encode ... | decode ...` on a corpus whose words are all listed prints what
`wakati` prints.  A line that is not a list of int32s ends the run with status 101, its line number on stderr and NOTHING on stdout, as `count` does.

`--normalize {none,nfc,nfkc}` (default none) on `tokenize`, `wakati`, `count`, `encode` and `graphviz`: the input -- INPUT, or stdin's lines with either
--split -- is normalised on the device first (include/kanpyo_gpu.h, "text normalisation"), and what is printed are the surfaces and words of the
NORMALISED text: half-width katakana, full-width letters and digits, U+3231 and the ideographic space then match the dictionary's keys.

`python -m kanpyo_amd normalize [INPUT] [-c DICT] [--form nfkc|nfc] [--split host|device]`: NOT a subcommand of the reference either -- the
normalised lines themselves, one output line per input line (kgpu_normalize_batch / kgpu_normalize_text).  Like every subcommand it needs a
dictionary: the device work runs on a dictionary handle's context pool.  A line that is not UTF-8 ends the run with status 101 as `wakati` does; a
line with an oversize segment prints unchanged, with a warning on stderr.

`python -m kanpyo_amd align [INPUT] [-c DICT] [--form nfkc|nfc]`: NOT a subcommand of the reference either -- an inspection tool for the source
alignment (include/kanpyo_gpu.h, "source alignment"): every line is normalised with its edit records, tokenized, and its token records are mapped back
to the line as it was given (kgpu_normalize_batch_aligned, kgpu_tokenize_batch, kgpu_source_spans_batch: all on the device); one output line per token,
`source_start\tsource_end\tsource surface\tnormalised surface` (character positions), and `EOS` behind each input line.  The text is formatted on
the host -- which needs the lines there: stdin's blocks are split on the host whatever --split says.  A line that is not UTF-8 ends the run with status 101.

`--sentences [--terminators CHARS] [--no-brackets]` on `tokenize`, `wakati`, `count`, `encode` and `normalize`: every line -- a paragraph, a document --
is cut into sentences on the device (include/kanpyo_gpu.h, "sentences": at 。｡！？!? outside matched brackets, or at CHARS) behind the normalisation
and in front of the subcommand's packed call, so one output line, or one EOS block, is printed per SENTENCE.  It goes with --nbest, --marginal, --sample
and --mode; not with `--split device` (the text calls split inside one C call), --offsets, --pair or --max-length, and not on `align` and `graphviz`.
"""
from __future__ import annotations

import argparse
import os
import sys
from functools import partial

import numpy as np

BLOCK_BYTES = 4 << 20     # stdin is read in blocks of about this many bytes, cut after the last newline
PANIC_STATUS = 101        # a Rust panic's exit status


def default_dict_path() -> str:
    """dirs::config_dir() on Linux ($XDG_CONFIG_HOME if absolute, else ~/.config) + kanpyo/ipa.dict (src/bin/kanpyo.rs:57-70)."""
    base = os.environ.get("XDG_CONFIG_HOME", "")
    if not os.path.isabs(base):
        base = os.path.join(os.path.expanduser("~"), ".config")
    return os.path.join(base, "kanpyo", "ipa.dict")


def _blocks(f, block_bytes: int):
    """Blocks of whole lines from a binary stream (the last one may lack its newline).  read1 returns what the stream has (a file: up to
    block_bytes; a pipe or a terminal: what has been written so far), so a line typed interactively is answered at once and a file still
    goes through in large blocks; more is read only while the block has no complete line or more input is already waiting."""
    import select

    buf = b""
    while True:
        chunk = f.read1(block_bytes)
        if not chunk:
            if buf:
                yield buf
            return
        buf += chunk
        while len(buf) < block_bytes and _ready(f, select):
            more = f.read1(block_bytes - len(buf))
            if not more:
                break
            buf += more
        cut = buf.rfind(b"\n") + 1
        if cut:
            yield buf[:cut]
            buf = buf[cut:]


def _ready(f, select) -> bool:
    try:
        return bool(select.select([f], [], [], 0)[0])
    except (OSError, ValueError, TypeError):   # (a stream without a file descriptor)
        return False


def _open(args):
    """The dictionary of -c (the default one without it) -> its Tokenizer, the display tables uploaded."""
    from . import dictfile
    from .tokenizer import Tokenizer

    df = dictfile.load_dict(args.custom_dict or default_dict_path())
    tok = Tokenizer(df.dict)
    tok.set_features(df.morph_feature_table, df.unk_feature_table)
    tok.dictfile = df   # (what renders records on the host reads the display tables here)
    return tok


def _results(args, stdin, packed_call, text_call):
    """One result per call over the input, in whichever of its three forms: packed_call(utf8, offsets) for the INPUT argument and for the
    blocks of stdin split on the host, text_call(block) for `--split device`."""
    if args.input is not None:   # that one string, untrimmed
        one = np.frombuffer(os.fsencode(args.input), dtype=np.uint8)
        return iter([packed_call(one, np.array([0, one.size], dtype=np.uint64))])
    if args.split == "device":   # the block as it was read: split, trimmed and all the rest on the device
        return (text_call(b) for b in _blocks(stdin, args.block_bytes))
    from .tokenizer import split_lines

    return (packed_call(*split_lines(b)) for b in _blocks(stdin, args.block_bytes))


def _sentence_form(args):
    """With --sentences the stage normalises, not the command: -> the form asked for (None: none), and the command's own is turned off."""
    if not getattr(args, "sentences", False):
        return None
    if args.command == "normalize":
        return args.form.upper()
    form, args.normalize = _form(args), "none"
    return form


def _sentence_stage(tok, args, form, call):
    """--sentences: call(utf8, offsets) over the lines' SENTENCES -- normalised first where --normalize (or `normalize`'s --form) asks for it, then cut on
    the device (Tokenizer.split_sentences_packed) -- so that every result has one entry per sentence.  A sentence's status is its own, and 4 where
    the normaliser left its line as it was.  form: _sentence_form's answer.  call=None: the sentences themselves (`normalize`)."""
    from .tokenizer import merge_status

    def packed(utf8, offs):
        nstatus = None
        if form:
            utf8, offs, nstatus = tok.normalize_packed(utf8, offs, form)
        text, soff, recs = tok.split_sentences_packed(utf8, offs, args.terminators, not args.no_brackets)
        if nstatus is not None:
            nstatus = nstatus[recs["line"].astype(np.int64)]
        if call is None:
            return text, soff, nstatus if nstatus is not None else np.zeros(len(recs), dtype=np.uint8)
        result = call(text, soff)
        if nstatus is not None:
            merge_status(result[-1] if isinstance(result, tuple) else result, nstatus)
        return result

    return packed


def _warn_unnormalized(status, line0: int) -> None:
    """One stderr line per line the normaliser left as it was (status 4: a segment too long), by its 1-based number."""
    for i in np.flatnonzero(status == 4).tolist():
        print(f"kanpyo_amd: line {line0 + i + 1}: a segment is too long to normalise (left unchanged)", file=sys.stderr)


def _print_lines(results, stdout, panic: str) -> int:
    """Each result's text as soon as it is there; a line that is not UTF-8 ends the run behind the lines before it."""
    line0 = 0
    for text, toff, status in results:
        bad = np.flatnonzero(status == 1)
        _warn_unnormalized(status[: int(bad[0])] if bad.size else status, line0)
        line0 += len(status)
        if bad.size:
            stdout.write(text[: int(toff[bad[0]])].tobytes())
            stdout.flush()
            print(panic, file=sys.stderr)
            return PANIC_STATUS
        stdout.write(text.tobytes())
        stdout.flush()
    return 0


def _each_checked(results, skip_invalid: bool, consume=None) -> int:
    """consume(result) for every result (a status array, or a tuple that ends with one) once its lines that are not UTF-8 have been reported
    on stderr by their 1-based numbers, which run on across the results; without --skip-invalid the first of them ends the run."""
    line0 = 0   # lines in the results before this one
    for r in results:
        status = r[-1] if isinstance(r, tuple) else r
        for i in np.flatnonzero(status == 1).tolist():
            print(f"kanpyo_amd: line {line0 + i + 1}: not valid UTF-8" + (" (skipped)" if skip_invalid else ""), file=sys.stderr)
            if not skip_invalid:
                return PANIC_STATUS
        _warn_unnormalized(status, line0)
        line0 += len(status)
        if consume is not None:
            consume(r)
    return 0


def _form(args):
    """--normalize as the binding's keyword: None, "NFC" or "NFKC"."""
    form = getattr(args, "normalize", "none")
    return None if form == "none" else form.upper()


def _nbest_lines(tok, n_best: int, form, utf8, offs):
    """tokenize_lines_packed's result with every line's n_best paths in place of its one: the paths from the device, their lines made here."""
    from .nbest import path_lines
    from .tokenizer import merge_status

    nstatus = None
    if form:
        utf8, offs, nstatus = tok.normalize_packed(utf8, offs, form)
    tokens, poff, toff, _, status = tok.tokenize_nbest_packed(utf8, offs, n_best)
    if nstatus is not None:
        merge_status(status, nstatus)
    raw, o, po, to = utf8.tobytes(), offs.tolist(), poff.tolist(), toff.tolist()
    known, unk = tok.dictfile.morph_feature_table, tok.dictfile.unk_feature_table
    out = [b"".join(path_lines(raw[o[i] : o[i + 1]], tokens[to[p] : to[p + 1]], known, unk) for p in range(po[i], po[i + 1])) for i in range(len(o) - 1)]
    loff = np.zeros(len(out) + 1, dtype=np.uint64)
    if out:
        loff[1:] = np.cumsum([len(x) for x in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), loff, status


def _prob_lines(tok, args, form, utf8, offs):
    """tokenize_lines_packed's result for --marginal (every line of `tokenize` -- or of every node, --all-morphs -- with its marginal appended) and for
    --sample N (every line's N sampled paths one after the other): the numbers and paths from the device, their lines made here."""
    from .nbest import path_lines
    from .prob import marginal_lines
    from .tokenizer import merge_status

    nstatus = None
    if form:
        utf8, offs, nstatus = tok.normalize_packed(utf8, offs, form)
    raw, o = utf8.tobytes(), offs.tolist()
    known, unk = tok.dictfile.morph_feature_table, tok.dictfile.unk_feature_table
    if args.marginal:
        tokens, probs, _, toff, _, _, status = tok.tokenize_marginals_packed(utf8, offs, args.theta, args.all_morphs, args.min_prob)
        to = toff.tolist()
        out = [marginal_lines(raw[o[i] : o[i + 1]], tokens[to[i] : to[i + 1]], probs[to[i] : to[i + 1]], known, unk) for i in range(len(o) - 1)]
    else:
        tokens, poff, toff, _, status = tok.tokenize_samples_packed(utf8, offs, args.sample, args.seed, args.theta)
        po, to = poff.tolist(), toff.tolist()
        out = [b"".join(path_lines(raw[o[i] : o[i + 1]], tokens[to[p] : to[p + 1]], known, unk) for p in range(po[i], po[i + 1])) for i in range(len(o) - 1)]
    if nstatus is not None:
        merge_status(status, nstatus)
    loff = np.zeros(len(out) + 1, dtype=np.uint64)
    if out:
        loff[1:] = np.cumsum([len(x) for x in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), loff, status


def _mode_lines(tok, mode: str, penalties, form, utf8, offs):
    """tokenize_lines_packed's result with every line's path under a mode's penalised costs: the records from the device, their lines made here."""
    from .nbest import path_lines
    from .tokenizer import merge_status

    nstatus = None
    if form:
        utf8, offs, nstatus = tok.normalize_packed(utf8, offs, form)
    tokens, toff, _, status = tok.tokenize_mode_packed(utf8, offs, mode, penalties)
    if nstatus is not None:
        merge_status(status, nstatus)
    raw, o, to = utf8.tobytes(), offs.tolist(), toff.tolist()
    known, unk = tok.dictfile.morph_feature_table, tok.dictfile.unk_feature_table
    out = [path_lines(raw[o[i] : o[i + 1]], tokens[to[i] : to[i + 1]], known, unk) for i in range(len(o) - 1)]
    loff = np.zeros(len(out) + 1, dtype=np.uint64)
    if out:
        loff[1:] = np.cumsum([len(x) for x in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), loff, status


def _user_lines(tok, userdict, mode, penalties, form, utf8, offs):
    """_mode_lines over the lattices widened by a user dictionary's matches (kgpu_tokenize_batch_user): a user token prints as its surface, a tab and
    the entry's features joined by commas."""
    from .nbest import path_lines
    from .tokenizer import merge_status

    nstatus = None
    if form:
        utf8, offs, nstatus = tok.normalize_packed(utf8, offs, form)
    tokens, toff, _, status = tok.tokenize_user_packed(utf8, offs, userdict, mode or "normal", penalties)
    if nstatus is not None:
        merge_status(status, nstatus)
    raw, o, to = utf8.tobytes(), offs.tolist(), toff.tolist()
    known, unk = tok.dictfile.morph_feature_table, tok.dictfile.unk_feature_table
    lines = []
    for i in range(len(o) - 1):
        line, recs, first, out = raw[o[i] : o[i + 1]], tokens[to[i] : to[i + 1]], 0, []
        for k in np.flatnonzero(recs["cls"] == 3).tolist() + [len(recs)]:   # (the runs between two user tokens are path_lines' to render)
            out.append(path_lines(line, recs[first:k], known, unk))
            if k < len(recs):
                pos, bl = int(recs[k]["position"]), int(recs[k]["byte_len"])
                out.append(line[pos : pos + bl] + b"\t" + ",".join(userdict.features(int(recs[k]["id"]))).encode("utf-8") + b"\n")
            first = k + 1
        lines.append(b"".join(out))
    loff = np.zeros(len(lines) + 1, dtype=np.uint64)
    if lines:
        loff[1:] = np.cumsum([len(x) for x in lines])
    return np.frombuffer(b"".join(lines), dtype=np.uint8), loff, status


def tokenize(args, stdin, stdout) -> int:
    tok = _open(args)
    sent_form = _sentence_form(args)
    packed, text = tok.tokenize_lines_packed, tok.tokenize_text_lines
    if getattr(args, "user_entries", None) is not None:
        from .userdict import UserDict

        userdict = UserDict(tok, args.user_entries)
        packed, text = partial(_user_lines, tok, userdict, args.mode, args.mode_penalties, _form(args)), None   # (parse_args refuses --split device)
    elif getattr(args, "mode", None) is not None:
        packed, text = partial(_mode_lines, tok, args.mode, args.mode_penalties, _form(args)), None   # (parse_args refuses --split device)
    elif getattr(args, "nbest", None) is not None:
        packed, text = partial(_nbest_lines, tok, args.nbest, _form(args)), None   # (parse_args refuses --split device)
    elif getattr(args, "marginal", False) or getattr(args, "sample", None) is not None:
        packed, text = partial(_prob_lines, tok, args, _form(args)), None          # (likewise)
    elif _form(args):
        packed, text = partial(packed, normalize=_form(args)), partial(text, normalize=_form(args))
    if args.sentences:
        packed, text = _sentence_stage(tok, args, sent_form, packed), None   # (parse_args refuses --split device)
    return _print_lines(_results(args, stdin, packed, text), stdout,
                        "thread 'main' panicked: failed to read from stdin: stream did not contain valid UTF-8")


def _words(args, **kw):
    """The Words handle of the command's field and filter; with --normalize it normalises whatever goes through it."""
    if _form(args):
        kw["normalize"] = _form(args)
    return _open(args).words(field=args.field, drop=args.drop, keep=args.keep, **kw)


def normalize(args, stdin, stdout) -> int:
    tok = _open(args)
    form = args.form.upper()
    line0 = 0
    packed, text = partial(tok.normalize_packed, form=form), partial(tok.normalize_text, form=form)
    if args.sentences:
        packed, text = _sentence_stage(tok, args, _sentence_form(args), None), None
    for text, toff, status in _results(args, stdin, packed, text):
        bad = np.flatnonzero(status == 1)
        shown = int(bad[0]) if bad.size else len(status)
        _warn_unnormalized(status[:shown], line0)
        raw, o = text.tobytes(), toff.tolist()
        stdout.write(b"".join(raw[o[i] : o[i + 1]] + b"\n" for i in range(shown)))
        stdout.flush()
        if bad.size:
            print("kanpyo_amd: failed to read from stdin: stream did not contain valid UTF-8", file=sys.stderr)
            return PANIC_STATUS
        line0 += len(status)
    return 0


def align(args, stdin, stdout) -> int:
    from .tokenizer import merge_status, split_lines

    tok = _open(args)
    form = args.form.upper()

    def packed(utf8, offs):
        text, ntoff, nstatus, edits, eoff = tok.normalize_packed_aligned(utf8, offs, form)
        tokens, toff, status = tok.tokenize_packed(text, ntoff)
        spans = tok.source_spans(tokens, toff, edits, eoff)
        merge_status(status, nstatus)
        src, norm, so, no, to = utf8.tobytes(), text.tobytes(), offs.tolist(), ntoff.tolist(), toff.tolist()
        out = []
        for i in range(len(status)):
            rows = []
            for k in range(to[i], to[i + 1] if status[i] != 1 else to[i]):
                t, sp = tokens[k], spans[k]
                if int(t["cls"]) == 0:   # the EOS dummy: the line below stands for it
                    continue
                s0, n0 = so[i] + int(sp["position"]), no[i] + int(t["position"])
                rows.append(b"%d\t%d\t" % (int(sp["start"]), int(sp["end"])) + src[s0 : s0 + int(sp["byte_len"])] + b"\t" + norm[n0 : n0 + int(t["byte_len"])] + b"\n")
            out.append(b"".join(rows) + b"EOS\n")
        loff = np.zeros(len(out) + 1, dtype=np.uint64)
        if out:
            loff[1:] = np.cumsum([len(x) for x in out])
        return np.frombuffer(b"".join(out), dtype=np.uint8), loff, status

    return _print_lines(_results(args, stdin, packed, lambda block: packed(*split_lines(block))), stdout,
                        "kanpyo_amd: failed to read from stdin: stream did not contain valid UTF-8")


def wakati(args, stdin, stdout) -> int:
    form = _sentence_form(args)
    w = _words(args, separator=os.fsencode(args.separator))
    packed = _sentence_stage(w.tokenizer, args, form, w.render_packed) if args.sentences else w.render_packed
    return _print_lines(_results(args, stdin, packed, w.render_text), stdout,
                        "kanpyo_amd: failed to read from stdin: stream did not contain valid UTF-8")


def count(args, stdin, stdout) -> int:
    form = _sentence_form(args)
    words = _words(args)
    counts = words.counter()
    packed = _sentence_stage(words.tokenizer, args, form, counts.add_packed) if args.sentences else counts.add_packed
    if _each_checked(_results(args, stdin, packed, counts.add_text), args.skip_invalid):
        return PANIC_STATUS   # nothing has been printed
    out = bytearray()
    for word, n in counts.most_common(args.top):
        out += b"%d\t" % n + word + b"\n"
    stdout.write(bytes(out))
    stdout.flush()
    return 0


def encode(args, stdin, stdout) -> int:
    if args.max_length is None and (args.stride is not None or args.truncation is not None or args.pair):
        print("kanpyo_amd: --stride, --truncation and --pair go with --max-length", file=sys.stderr)
        return 2
    if args.max_length is not None and (args.offsets or args.bos is None or args.eos is None):
        print("kanpyo_amd: --max-length needs --bos and --eos (the rows' specials) and does not go with --offsets", file=sys.stderr)
        return 2
    if args.offsets or args.max_length is not None:   # (encode_tensor's tensors: torch ships its own HIP runtime, which has to be the process's one -- loaded before the library is)
        import torch  # noqa: F401
    from .vocab import Vocab

    try:
        listed = Vocab.read_words(args.vocab)
    except OSError as e:
        print(f"kanpyo_amd: --vocab: {e}", file=sys.stderr)
        return 2
    have = set(listed)
    for opt, word in (("--unk", args.unk), ("--bos", args.bos), ("--eos", args.eos)):
        if word is not None and os.fsencode(word) not in have:
            print(f"kanpyo_amd: {opt} {word!r} is not a line of {args.vocab}", file=sys.stderr)
            return 2
    enc = lambda w: None if w is None else os.fsencode(w)   # noqa: E731
    if not args.wordpiece and (args.prefix is not None or args.max_word_chars is not None):
        print("kanpyo_amd: --prefix and --max-word-chars go with --wordpiece", file=sys.stderr)
        return 2
    wp = {}
    if args.wordpiece:
        wp = dict(wordpiece=True, prefix=os.fsencode("##" if args.prefix is None else args.prefix), max_word_chars=100 if args.max_word_chars is None else args.max_word_chars)
        if len(wp["prefix"]) > 8 or wp["max_word_chars"] > 1024:
            print("kanpyo_amd: --prefix has at most 8 bytes, --max-word-chars is at most 1024", file=sys.stderr)
            return 2
    form = _sentence_form(args)
    v = Vocab.from_words(_words(args), listed, enc(args.unk), enc(args.bos), enc(args.eos), **wp)
    out = bytearray()   # (nothing is printed before the input is known to be valid, or --skip-invalid says not to care)

    def with_offsets(utf8, offs):
        src, so = utf8.tobytes(), offs.tolist()
        ids, ioff, status, spans, tix = v.encode_tensor([src[so[i] : so[i + 1]] for i in range(len(so) - 1)], return_spans=True)
        ids, sp, tix, o = ids.cpu().tolist(), spans.cpu().numpy().view(np.uint32).tolist(), tix.cpu().tolist(), ioff.cpu().tolist()
        lines = []
        for i in range(len(so) - 1):
            rows = [b"%d\t%d\t%d\t%d\t" % (ids[e], sp[e][2], sp[e][3], tix[e]) + src[so[i] + sp[e][0] : so[i] + sp[e][0] + sp[e][1]] + b"\n" for e in range(o[i], o[i + 1])]
            lines.append(b"".join(rows) + b"EOS\n")
        return lines, status.cpu().numpy()

    line0 = [0]   # input lines in the blocks before this one: the rows' sample numbers run on

    def model_rows(utf8, offs):
        src, so = utf8.tobytes(), offs.tolist()
        lines = [src[so[i] : so[i + 1]] for i in range(len(so) - 1)]
        first, second = lines, None
        if args.pair:
            cut = [ln.partition(b"\t") for ln in lines]
            first, second = [c[0] for c in cut], [c[2] for c in cut]
        r = v.encode_pairs_tensor(first, second, max_length=args.max_length, stride=args.stride or 0, truncation=args.truncation or "only_second")
        ids, mask, sample = r["input_ids"].cpu().numpy(), r["attention_mask"].cpu().numpy(), r["sample_of_row"].cpu().tolist()
        rows = [b"%d\t" % (line0[0] + sample[k]) + " ".join(map(str, ids[k][mask[k] == 1].tolist())).encode() + b"\n" for k in range(ids.shape[0])]
        line0[0] += len(lines)
        st = r["sentence_status"].cpu().numpy()
        return rows, (np.maximum(st[: len(lines)], st[len(lines):]) if args.pair else st)

    def listing(result):
        out.extend(b"".join(result[0]))
        if args.skip_invalid:
            stdout.write(bytes(out))
            stdout.flush()
            out.clear()

    def decimal(result):
        ids, ioff, _ = result
        o, dec = ioff.tolist(), ids.tolist()
        out.extend("".join(" ".join(map(str, dec[o[i] : o[i + 1]])) + "\n" for i in range(len(o) - 1)).encode())
        if args.skip_invalid:
            stdout.write(bytes(out))
            stdout.flush()
            out.clear()

    if args.offsets or args.max_length is not None:
        from .tokenizer import split_lines

        call = with_offsets if args.offsets else model_rows
        results = _results(args, stdin, call, lambda block: call(*split_lines(block)))
    else:
        packed = _sentence_stage(v._open_tokenizer(), args, form, v.encode_packed) if args.sentences else v.encode_packed
        results = _results(args, stdin, packed, v.encode_text)
    if _each_checked(results, args.skip_invalid, listing if args.offsets or args.max_length is not None else decimal):
        return PANIC_STATUS   # nothing has been printed
    stdout.write(bytes(out))
    stdout.flush()
    return 0


def parse_id_lines(data: bytes):
    """Lines of decimal int32s separated by blanks (what `encode` prints) -> (ids int32, offsets uint64 [lines + 1]), or the 1-based number of the
    first line that is something else.  The last line may lack its newline; an empty line is the empty sequence."""
    rows = data.split(b"\n")
    if rows and rows[-1] == b"":
        rows.pop()
    ids, offs = [], [0]
    for k, row in enumerate(rows):
        try:
            vals = [int(t) for t in row.split()]
        except ValueError:
            return k + 1
        if any(not -2**31 <= v < 2**31 for v in vals) or not row.isascii() or b"_" in row:
            return k + 1
        ids += vals
        offs.append(len(ids))
    return np.array(ids, dtype=np.int64).astype(np.int32), np.array(offs, dtype=np.uint64)


def decode(args, stdin, stdout) -> int:
    from .vocab import Vocab

    try:
        listed = Vocab.read_words(args.vocab)
    except OSError as e:
        print(f"kanpyo_amd: --vocab: {e}", file=sys.stderr)
        return 2
    if not args.wordpiece and args.prefix is not None:
        print("kanpyo_amd: --prefix goes with --wordpiece", file=sys.stderr)
        return 2
    wp = {}
    if args.wordpiece:
        wp = dict(wordpiece=True, prefix=os.fsencode("##" if args.prefix is None else args.prefix))
        if len(wp["prefix"]) > 8:
            print("kanpyo_amd: --prefix has at most 8 bytes", file=sys.stderr)
            return 2
    # (the ids stand for themselves: no word of the list is special here, and unk_id only has to be an id)
    v = Vocab(_open(args).words(), listed, 0, **wp)
    sep = os.fsencode(args.separator)
    out = bytearray()   # (nothing is printed before the input is known to be lists of ids)
    line0 = 0
    blocks = [os.fsencode(args.input)] if args.input is not None else _blocks(stdin, args.block_bytes)
    for block in blocks:
        parsed = parse_id_lines(block)
        if isinstance(parsed, int):
            print(f"kanpyo_amd: line {line0 + parsed}: not a list of int32 ids", file=sys.stderr)
            return PANIC_STATUS
        ids, offs = parsed
        line0 += offs.size - 1
        o = offs.tolist()
        out += b"".join(ln + b"\n" for ln in v.decode([ids[o[i] : o[i + 1]] for i in range(len(o) - 1)], separator=sep, skip=args.skip))
    stdout.write(bytes(out))
    stdout.flush()
    return 0


def _skip_list(text: str):
    """--skip: at most 8 int32 ids separated by commas."""
    try:
        ids = [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid skip list {text!r}: ids separated by commas")
    if len(ids) > 8 or any(not -2**31 <= k < 2**31 for k in ids):
        raise argparse.ArgumentTypeError(f"invalid skip list {text!r}: at most 8 ids, each an int32")
    return ids


def _decode_separator(text: str) -> str:
    if len(text.encode("utf-8", "surrogateescape")) > 8:
        raise argparse.ArgumentTypeError(f"invalid separator {text!r}: at most 8 bytes")
    return text


def _nbest(text: str) -> int:
    if not text.isascii() or not text.isdigit() or not 1 <= int(text) <= 64:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: a number of paths from 1 to 64")
    return int(text)


def _mode_penalties(text: str):
    """--mode-penalties KL,KP,OL,OP: four unsigned 32-bit numbers."""
    parts = text.split(",")
    if len(parts) != 4 or not all(v.isascii() and v.isdigit() and int(v) < 1 << 32 for v in parts):
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: KL,KP,OL,OP -- kanji length, kanji penalty, other length, other penalty, each below 2^32")
    return tuple(int(v) for v in parts)


def _sample(text: str) -> int:
    if not text.isascii() or not text.isdigit() or not 1 <= int(text) <= 256:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: a number of samples from 1 to 256")
    return int(text)


def _seed(text: str) -> int:
    if not text.isascii() or not text.isdigit() or int(text) >= 1 << 64:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: an unsigned integer below 2^64")
    return int(text)


def _theta(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        v = 0.0
    if not 0.0 < v <= 2.0**64:   # KGPU_THETA_MAX
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: a number above 0 and at most 2^64")
    return v


def _min_prob(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        v = -1.0
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: a probability from 0 to 1")
    return v


def _terminators(text: str) -> str:
    if not 1 <= len(text) <= 16:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: 1 to 16 characters")
    return text


def _top(text: str) -> int:
    if not text.isascii() or not text.isdigit() or int(text) < 1:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: a count from 1")
    return int(text)


def _pos_list(text: str):
    """--drop / --keep: part-of-speech names separated by commas."""
    return [p for p in text.split(",") if p]


def _separator(text: str) -> str:
    b = text.encode("utf-8", "surrogateescape")
    if len(b) != 1 or b == b"\n":
        raise argparse.ArgumentTypeError(f"invalid separator {text!r}: one byte, not a newline")
    return text


def _field(text: str) -> int:
    if not text.isascii() or not text.isdigit():
        raise argparse.ArgumentTypeError(f"invalid field {text!r}: a feature index from 0")
    return int(text)


# what Rust's str::trim_end strips: the Unicode White_Space code points (char::is_whitespace)
WHITE_SPACE = "\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000"


def first_line(data: bytes) -> bytes:
    """What `kanpyo graphviz` draws when stdin holds `data` (src/bin/kanpyo.rs:134-143): read_line takes the bytes up to and including the
    first '\n' (all of them if there is none) and fails unless they are UTF-8 (UnicodeDecodeError here); trim_end strips the trailing
    White_Space.  The lines behind the first are never read."""
    cut = data.find(b"\n") + 1
    line = data[:cut] if cut else data
    return line.decode("utf-8").rstrip(WHITE_SPACE).encode("utf-8")


def graphviz(args, stdin, stdout) -> int:
    if args.input is not None:   # that one string, untrimmed
        raw = os.fsencode(args.input)
    else:
        try:
            raw = first_line(stdin.readline())
        except UnicodeDecodeError:
            print("thread 'main' panicked: failed to read from stdin: stream did not contain valid UTF-8", file=sys.stderr)
            return PANIC_STATUS
    one, offs = np.frombuffer(raw, dtype=np.uint8), np.array([0, len(raw)], dtype=np.uint64)
    tok = _open(args)
    if _form(args):   # the lattice of the normalised sentence
        one, offs, _ = tok.normalize_packed(one, offs, _form(args))
    text, _, status = tok.graphviz_packed(one, offs, dpi=args.dpi, full_state=args.full_state)
    if status[0]:   # (an INPUT argument that is not UTF-8: the reference's argument parser rejects it)
        print(f"kanpyo_amd: the input cannot be drawn (sentence status {int(status[0])})", file=sys.stderr)
        return 2
    stdout.write(text.tobytes())
    stdout.flush()
    return 0


def _dpi(text: str) -> int:
    """--dpi is a usize in the reference (src/bin/kanpyo.rs:45-47): a decimal in 0 .. 2^64 - 1, nothing else."""
    digits = text[1:] if text.startswith("+") else text   # (usize::from_str takes a leading '+')
    if not digits.isascii() or not digits.isdigit() or int(digits) >= 1 << 64:
        raise argparse.ArgumentTypeError(f"invalid value {text!r}: an unsigned integer below 2^64")
    return int(digits)


NORMALIZE_CHOICES = ["none", "nfc", "nfkc"]
NORMALIZE_HELP = "Normalise the input on the device first: the output refers to the normalised text [default: none]"


def _text_command(sub, name: str, help: str, verb: str = None, first=(), own=(), skip_invalid: str = None):
    """A subcommand over lines of text: INPUT or stdin, the dictionary, where the blocks are split; with `verb` ("Print", ...) wakati's field and
    filter as well.  first / own: the command's own options as (flag, keywords), listed in front of / behind those; skip_invalid: its help."""
    p = sub.add_parser(name, help=help)
    p.add_argument("input", nargs="?", default=None, help="Input text to analyze [default: stdin]")
    p.add_argument("-d", "--dict", choices=["ipa"], default="ipa", help="Dictionary")
    p.add_argument("-c", "--custom-dict", default=None, help="Custom dictionary (.dict)")
    for flag, kw in first:
        p.add_argument(flag, **kw)
    if verb:
        fld = p.add_mutually_exclusive_group()
        fld.add_argument("--field", type=_field, default=None, help=f"{verb} feature N of the token's row instead of the surface")
        fld.add_argument("--base-form", dest="field", action="store_const", const=6, help="--field 6 (IPADIC)")
        fld.add_argument("--reading", dest="field", action="store_const", const=7, help="--field 7 (IPADIC)")
        fld.add_argument("--pronunciation", dest="field", action="store_const", const=8, help="--field 8 (IPADIC)")
        flt = p.add_mutually_exclusive_group()
        flt.add_argument("--drop", type=_pos_list, default=[], help="Drop tokens whose part of speech (feature 0) is one of POS[,POS...]")
        flt.add_argument("--keep", type=_pos_list, default=[], help="Keep only tokens whose part of speech is one of POS[,POS...]")
    for flag, kw in own:
        p.add_argument(flag, **kw)
    if name not in ("normalize", "align"):
        p.add_argument("--normalize", choices=NORMALIZE_CHOICES, default="none", help=NORMALIZE_HELP)
    if name != "align":
        p.add_argument("--sentences", action="store_true",
                       help="Cut every line into sentences on the device first, behind the normalisation: at 。｡！？!? outside brackets; one output line (or EOS block) per sentence")
        p.add_argument("--terminators", type=_terminators, default=None, metavar="CHARS", help="With --sentences: the characters a sentence ends at, at most 16 [default: 。｡！？!?]")
        p.add_argument("--no-brackets", action="store_true", help="With --sentences: a terminator inside brackets ends a sentence too")
    p.add_argument("--split", choices=["host", "device"], default="host",
                   help="Where stdin's blocks are split into lines and trimmed [default: host]")
    if skip_invalid:
        p.add_argument("--skip-invalid", action="store_true", help=skip_invalid)
    p.add_argument("--block-bytes", type=int, default=BLOCK_BYTES, help=argparse.SUPPRESS)
    return p


def _prob_defaults(args):
    """The documented defaults of --min-prob, --seed and --theta (None on the command line: not given, which parse_args tells apart)."""
    from ._lib import KGPU_THETA_DEFAULT

    args.min_prob = 0.0 if args.min_prob is None else args.min_prob
    args.seed = 0 if args.seed is None else args.seed
    args.theta = KGPU_THETA_DEFAULT if args.theta is None else args.theta


def parse_args(argv=None):
    """The reference's command line (src/bin/kanpyo.rs:14-49).  -> the namespace; .command is "tokenize" or "graphviz" -- or "wakati", "count", "encode", "normalize" or "align", which are this package's own."""
    p = argparse.ArgumentParser(prog="kanpyo_amd", description="Japanese Morphological Analyzer (kanpyo) on AMD Instinct GPUs")
    sub = p.add_subparsers(dest="command")
    t = _text_command(sub, "tokenize", "Tokenize input text",
                      own=[("--nbest", dict(type=_nbest, default=None, metavar="K", help="Print each line's K lowest-cost paths, best first (1..64; not in the reference: mecab -N K)")),
                           ("--marginal", dict(action="store_true", help="Append each token's marginal probability to its line (not in the reference: mecab -m)")),
                           ("--all-morphs", dict(action="store_true", help="With --marginal: a line for every node of the lattice, not only the best path's (mecab -a)")),
                           ("--min-prob", dict(type=_min_prob, default=None, metavar="P", help="With --marginal --all-morphs: only the nodes whose marginal is at least P [default: 0]")),
                           ("--sample", dict(type=_sample, default=None, metavar="N", help="Print N tokenizations of each line drawn from the lattice (1..256; not in the reference: mecab -l)")),
                           ("--seed", dict(type=_seed, default=None, metavar="S", help="With --sample: the seed of the draws [default: 0]")),
                           ("--theta", dict(type=_theta, default=None, metavar="T", help="With --marginal / --sample: P(path) is proportional to exp(-T cost) [default: 0.75 / 800]")),
                           ("--mode", dict(choices=["normal", "search", "extended"], default=None, help="search: a length penalty on long words splits compounds into the parts the dictionary has; extended: unknown words are also cut into characters; normal: what tokenize prints (not in the reference)")),
                           ("--mode-penalties", dict(type=_mode_penalties, default=None, metavar="KL,KP,OL,OP", help="With --mode: kanji length, kanji penalty, other length, other penalty [default: 2,3000,7,1700]")),
                           ("--user-dict", dict(default=None, metavar="FILE", help="Extra words beside the dictionary's: a MeCab user CSV, surface,left_id,right_id,cost,feature,... per line; a user token prints its surface and the entry's features (not in the reference: mecab -u)"))])
    g = sub.add_parser("graphviz", help="Output lattice in Graphviz format")
    g.add_argument("input", nargs="?", default=None, help="Input text to analyze [default: one line of stdin]")
    g.add_argument("-d", "--dict", choices=["ipa"], default="ipa", help="Dictionary")
    g.add_argument("-c", "--custom-dict", default=None, help="Custom dictionary (.dict)")
    g.add_argument("-f", "--full-state", action="store_true", help="Output full state of lattice")
    g.add_argument("--dpi", type=_dpi, default=48, help="DPI of output image [default: 48]")
    g.add_argument("--normalize", choices=NORMALIZE_CHOICES, default="none", help=NORMALIZE_HELP)
    _text_command(sub, "normalize", "NFC / NFKC of each input line (not in the reference)",
                  own=[("--form", dict(choices=["nfkc", "nfc"], default="nfkc", help="The normalisation form [default: nfkc]"))])
    _text_command(sub, "align", "Each token's place in the line as it was given, through NFC / NFKC (not in the reference)",
                  own=[("--form", dict(choices=["nfkc", "nfc"], default="nfkc", help="The normalisation form [default: nfkc]"))])
    _text_command(sub, "wakati", "One line of separated words per input line (not in the reference)", "Print",
                  own=[("--separator", dict(type=_separator, default=" ", help="The byte between words [default: a space]"))])
    _text_command(sub, "count", "Word frequencies of the whole input (not in the reference)", "Count",
                  own=[("--top", dict(type=_top, default=None, help="Print the N most frequent words only"))],
                  skip_invalid="Skip lines that are not UTF-8 instead of ending with status 101")
    _text_command(sub, "encode", "Vocabulary ids of each input line's words (not in the reference)", "Encode",
                  first=[("--vocab", dict(required=True, help="The vocabulary: one word per line, line k (0-based) is id k"))],
                  own=[("--unk", dict(default="<unk>", help="The word of the vocabulary whose id a word outside it gets [default: <unk>]")),
                       ("--bos", dict(default=None, help="A word of the vocabulary whose id goes in front of every line's ids")),
                       ("--eos", dict(default=None, help="A word of the vocabulary whose id goes behind every line's ids")),
                       ("--wordpiece", dict(action="store_true", help="The vocabulary is a WordPiece list (a BERT vocab.txt): a word outside it is cut into its longest listed pieces")),
                       ("--prefix", dict(default=None, help="With --wordpiece: the continuation prefix, at most 8 bytes [default: ##]")),
                       ("--max-word-chars", dict(type=_top, default=None, help="With --wordpiece: a longer word gets the --unk id [default: 100]")),
                       ("--offsets", dict(action="store_true", help="One output line per id: id, start, end (characters of the line as given), token index, text; EOS behind each input line")),
                       ("--max-length", dict(type=_top, default=None, help="Print model input rows of at most N ids, specials included: one line per row, the input line's number and the ids up to the pad")),
                       ("--stride", dict(type=_field, default=None, help="With --max-length: the ids consecutive windows of a cut line share [default: 0]")),
                       ("--truncation", dict(choices=["only_second", "only_first", "longest_first"], default=None, help="With --max-length: which side is cut [default: only_second]")),
                       ("--pair", dict(action="store_true", help="With --max-length: an input line is a<TAB>b, a sentence pair"))],
                  skip_invalid="A line that is not UTF-8 prints its bos / eos only instead of ending the run with status 101")
    dc = sub.add_parser("decode", help="The words of each input line's vocabulary ids, joined (not in the reference)")
    dc.add_argument("input", nargs="?", default=None, help="Ids to decode: decimal numbers separated by spaces [default: stdin, one sequence per line]")
    dc.add_argument("-d", "--dict", choices=["ipa"], default="ipa", help="Dictionary")
    dc.add_argument("-c", "--custom-dict", default=None, help="Custom dictionary (.dict)")
    dc.add_argument("--vocab", required=True, help="The vocabulary: one word per line, line k (0-based) is id k")
    dc.add_argument("--wordpiece", action="store_true", help="The vocabulary is a WordPiece list: a continuation piece joins the word in front of it without its prefix")
    dc.add_argument("--prefix", default=None, help="With --wordpiece: the continuation prefix, at most 8 bytes [default: ##]")
    dc.add_argument("--separator", type=_decode_separator, default=" ", help="What stands between words, 0 to 8 bytes [default: a space]")
    dc.add_argument("--skip", type=_skip_list, default=[], help="Ids that give no text: ID[,ID...], at most 8")
    dc.add_argument("--block-bytes", type=int, default=BLOCK_BYTES, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.command == "tokenize" and args.nbest is not None and args.split == "device":
        t.error("--nbest renders its lines on the host: it does not go with --split device")
    if args.command == "tokenize":
        prob = args.marginal or args.sample is not None
        if args.marginal and args.sample is not None:
            t.error("--marginal and --sample are two outputs: one of them")
        if prob and args.nbest is not None:
            t.error("--marginal / --sample do not go with --nbest")
        if prob and args.split == "device":
            t.error("--marginal / --sample render their lines on the host: they do not go with --split device")
        if (args.all_morphs or args.min_prob is not None) and not args.marginal:
            t.error("--all-morphs / --min-prob go with --marginal")
        if args.seed is not None and args.sample is None:
            t.error("--seed goes with --sample")
        if args.theta is not None and not prob:
            t.error("--theta goes with --marginal or --sample")
        if args.mode is not None and (prob or args.nbest is not None):
            t.error("--mode does not go with --nbest, --marginal or --sample")
        if args.mode is not None and args.split == "device":
            t.error("--mode renders its lines on the host: it does not go with --split device")
        if args.mode_penalties is not None and args.mode is None:
            t.error("--mode-penalties goes with --mode")
        args.user_entries = None
        if args.user_dict is not None:
            if prob or args.nbest is not None:
                t.error("--user-dict does not go with --nbest, --marginal or --sample")
            if args.split == "device":
                t.error("--user-dict renders its lines on the host: it does not go with --split device")
            from .userdict import UserDictFormatError, parse_csv

            try:
                with open(args.user_dict, encoding="utf-8", newline="") as f:
                    args.user_entries = parse_csv(f.read(), _form(args))
            except (OSError, UnicodeDecodeError) as e:
                t.error(f"--user-dict {args.user_dict}: {e}")
            except UserDictFormatError as e:
                t.error(f"--user-dict {args.user_dict}: {e}")
        _prob_defaults(args)
    if getattr(args, "sentences", False):
        if args.split == "device":
            p.error("--sentences works on packed lines: it does not go with --split device (the text calls split inside one C call)")
        if getattr(args, "offsets", False) or getattr(args, "pair", False) or getattr(args, "max_length", None) is not None:
            p.error("--sentences does not go with --offsets, --pair or --max-length")
    elif getattr(args, "terminators", None) is not None or getattr(args, "no_brackets", False):
        p.error("--terminators and --no-brackets go with --sentences")
    if args.command is None:   # src/bin/kanpyo.rs:173: no subcommand == tokenize from stdin, default dictionary
        args = t.parse_args([])
        args.command = "tokenize"
        _prob_defaults(args)
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    from . import _lib

    try:
        if args.command == "graphviz":
            return graphviz(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "wakati":
            return wakati(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "count":
            return count(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "encode":
            return encode(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "decode":
            return decode(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "normalize":
            return normalize(args, sys.stdin.buffer, sys.stdout.buffer)
        if args.command == "align":
            return align(args, sys.stdin.buffer, sys.stdout.buffer)
        return tokenize(args, sys.stdin.buffer, sys.stdout.buffer)
    except _lib.KgpuError as e:
        print(f"kanpyo_amd: {e}", file=sys.stderr)
        return 1
