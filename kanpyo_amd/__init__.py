"""kanpyo_amd -- MI355X-native drop-in for kanpyo::Tokenizer::tokenize().

Host-side mirror of the reference's public API for that one path
(src/tokenizer.rs, src/token.rs) over the C ABI of libkanpyo_gpu.so
(include/kanpyo_gpu.h).  The HIP extension is mandatory: there is no CPU
fallback, importing the tokenizer without the built library raises.
"""
from .token import AlignedToken, NBestPath, Token, TokenClass  # noqa: F401
from .dict import Dict  # noqa: F401
from .tokenizer import Tokenizer, TOKEN_DTYPE, normalize_host, normalize_host_aligned, split_sentences_host, SENTENCE_DTYPE  # noqa: F401
from .vocab import Vocab  # noqa: F401
from .pack import pack_host  # noqa: F401
from .decode import decode_host  # noqa: F401
from .nbest import nbest_host  # noqa: F401
from .prob import marginals_host, samples_host  # noqa: F401
from .mode import mode_host  # noqa: F401
from .userdict import UserDict, UserEntry, userdict_host  # noqa: F401

__all__ = ["AlignedToken", "Token", "TokenClass", "Dict", "Tokenizer", "TOKEN_DTYPE", "Vocab", "normalize_host", "normalize_host_aligned", "split_sentences_host", "SENTENCE_DTYPE", "pack_host", "decode_host", "NBestPath", "nbest_host", "marginals_host", "samples_host", "mode_host", "UserDict", "UserEntry", "userdict_host"]
