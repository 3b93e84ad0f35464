"""Token / TokenClass (reference src/token.rs:3-55)."""
from __future__ import annotations

import enum
from dataclasses import dataclass


class TokenClass(enum.IntEnum):
    """src/token.rs:3-8.  Integer values are the C ABI's KGPU_CLASS_*."""

    Dummy = 0
    Known = 1
    Unknown = 2
    User = 3   # a user dictionary's entry (include/kanpyo_gpu.h, "user dictionary"; not in the reference): Token.id is the entry's index + 1
    USER = 3


@dataclass(frozen=True)
class Token:
    """src/token.rs:10-18; equality compares all six fields (src/token.rs:44-53)."""

    id: int
    class_: TokenClass
    position: int  # byte position
    start: int  # char position
    end: int  # char position
    surface: str

    def length(self) -> int:  # src/token.rs:39-41
        return self.end - self.start


@dataclass(frozen=True)
class AlignedToken:
    """A token of NORMALISED text with its place in the text the caller supplied (include/kanpyo_gpu.h, "source alignment"; not in the reference).
    token: what tokenize_batch(normalize=...) returns; source_*: kgpu_span's position, byte_len, start and end; source_surface: the source bytes
    the span covers ("EOS" for the dummy) -- every normalised character of a changed segment maps to the whole source segment."""

    token: Token
    source_position: int  # byte position in the source sentence
    source_byte_len: int
    source_start: int  # char position
    source_end: int  # char position
    source_surface: str


@dataclass(frozen=True)
class NBestPath:
    """One of a sentence's N-best paths (include/kanpyo_gpu.h, "N-best paths"; not in the reference): its total cost and its tokens, the Token
    objects tokenize_batch gives -- EOS last."""

    cost: int
    tokens: tuple
