"""`python -m kanpyo_amd tokenize [-c DICT] [INPUT]`: the reference's `kanpyo tokenize` (src/bin/kanpyo.rs:106-126, 174-197) on the device.

Its stdout is the reference binary's, byte for byte: one `surface\\tf1,f2,...` line per token, sentences one after the other.  With INPUT
that one string is tokenized untrimmed; without it stdin is read line by line (split at '\\n', trailing Unicode White_Space trimmed, as
read_line + trim_end do) -- here in blocks of whole lines, each tokenized and rendered on the device in one kgpu_tokenize_batch_lines
call and written out as soon as it is done.  `--split device` hands each block to kgpu_tokenize_text_lines as it was read: the split and the
trim run on the device too (`--split host`, the default, splits with kgpu_split_lines on the host).  A line that is not UTF-8 ends the
run as the reference's `expect` panic does: the lines before it are printed, exit status 101.  No subcommand means `tokenize` from stdin.  The `graphviz` subcommand is not served.
"""
from __future__ import annotations

import argparse
import os
import sys

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


def tokenize(args, stdin, stdout) -> int:
    from . import dictfile
    from .tokenizer import Tokenizer, split_lines

    df = dictfile.load_dict(args.custom_dict or default_dict_path())
    tok = Tokenizer(df.dict)
    tok.set_features(df.morph_feature_table, df.unk_feature_table)
    if args.input is not None:   # that one string, untrimmed
        one = np.frombuffer(os.fsencode(args.input), dtype=np.uint8)
        results = iter([tok.tokenize_lines_packed(one, np.array([0, one.size], dtype=np.uint64))])
    elif args.split == "device":   # the block as it was read: split, trimmed, tokenized and rendered on the device
        results = (tok.tokenize_text_lines(b) for b in _blocks(stdin, args.block_bytes))
    else:
        results = (tok.tokenize_lines_packed(*split_lines(b)) for b in _blocks(stdin, args.block_bytes))
    for text, toff, status in results:
        bad = np.flatnonzero(status == 1)
        if bad.size:
            stdout.write(text[: int(toff[bad[0]])].tobytes())
            stdout.flush()
            print("thread 'main' panicked: failed to read from stdin: stream did not contain valid UTF-8", file=sys.stderr)
            return PANIC_STATUS
        stdout.write(text.tobytes())
        stdout.flush()
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="kanpyo_amd", description="Japanese Morphological Analyzer (kanpyo) on AMD Instinct GPUs")
    sub = p.add_subparsers(dest="command")
    t = sub.add_parser("tokenize", help="Tokenize input text")
    t.add_argument("input", nargs="?", default=None, help="Input text to analyze [default: stdin]")
    t.add_argument("-d", "--dict", choices=["ipa"], default="ipa", help="Dictionary")
    t.add_argument("-c", "--custom-dict", default=None, help="Custom dictionary (.dict)")
    t.add_argument("--split", choices=["host", "device"], default="host",
                   help="Where stdin's blocks are split into lines and trimmed [default: host]")
    t.add_argument("--block-bytes", type=int, default=BLOCK_BYTES, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.command is None:   # src/bin/kanpyo.rs:173: no subcommand == tokenize from stdin, default dictionary
        args = t.parse_args([])
    from . import _lib

    try:
        return tokenize(args, sys.stdin.buffer, sys.stdout.buffer)
    except _lib.KgpuError as e:
        print(f"kanpyo_amd: {e}", file=sys.stderr)
        return 1
