"""kgpu_dict_set_features checks feature ids only in the rows a token can name (rows 1..n_morphs of morph_feature.dict, 1..n_unk of the
unknown table): print_tokens (src/bin/kanpyo.rs:178-188) never indexes the others, so a table with extra rows loads as it does in the
reference, whatever those rows hold.  Through the host-only kgpu_debug_feature_pool hook (no device)."""
import ctypes as C

import numpy as np

from kanpyo_amd import _lib
from kanpyo_amd.dictfile import MorphFeatureTable


def _pool(known: MorphFeatureTable, unk: MorphFeatureTable, n_morphs: int, n_unk: int):
    a, b = np.frombuffer(known.encode(), dtype=np.uint8), np.frombuffer(unk.encode(), dtype=np.uint8)
    off = np.zeros(n_morphs + n_unk + 1, dtype=np.uint32)
    pool = np.zeros(256, dtype=np.uint8)
    got = C.c_uint64(0)
    rc = _lib.lib().kgpu_debug_feature_pool(a.ctypes.data, a.size, b.ctypes.data, b.size, n_morphs, n_unk, pool.ctypes.data, pool.size,
                                            off.ctypes.data, C.byref(got))
    return rc, pool[: got.value].tobytes(), off.tolist()


def test_rows_past_the_morphs_are_not_checked():
    unk = MorphFeatureTable([[1]], ["", "u"])
    rc, pool, off = _pool(MorphFeatureTable([[1], [2], [9]], ["", "a", "b"]), unk, 2, 1)
    assert rc == _lib.KGPU_OK, _lib.lib().kgpu_last_error()
    assert pool == b"abu" and off == [0, 1, 2, 3]
    rc, pool, off = _pool(MorphFeatureTable([[1]], ["", "a"]), MorphFeatureTable([[1], [7, 8]], ["", "u"]), 1, 1)
    assert rc == _lib.KGPU_OK and pool == b"au"


def test_a_nameable_row_is_still_checked():
    unk = MorphFeatureTable([[1]], ["", "u"])
    rc, _, _ = _pool(MorphFeatureTable([[1], [2], [9]], ["", "a", "b"]), unk, 3, 1)
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:181" in _lib.lib().kgpu_last_error().decode()
    rc, _, _ = _pool(MorphFeatureTable([[1]], ["", "a"]), MorphFeatureTable([[1], [7]], ["", "u"]), 1, 2)
    assert rc == _lib.KGPU_ERR_BAD_DICT and "kanpyo.rs:188" in _lib.lib().kgpu_last_error().decode()
