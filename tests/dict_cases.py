"""Hand-made dictionaries and lattices that a CPU test derives answers for and a GPU test runs on the device: the non-square and saturating
connection matrices (tests/test_matrix_cpu.py, tests/test_gpu_matrix.py, tests/test_gpu_graphviz.py), the naive restatement's lattice as a
kanpyo_amd.lattice.Lattice (tests/test_lattice_cpu.py; the device dumps of test_gpu_matrix / test_gpu_graphviz / test_gpu_parity are compared with it)
and a tiny MeCab-format source directory (tests/test_builder_cpu.py, test_gpu_parity's built-and-reloaded dictionary).  Imports without a device."""
import numpy as np

from conftest import fixture_dict_parts

A, I = "あ", "い"


# ------------------------------------------------------------------------------------------------------------------------- connection matrices
def saturation_parts():
    """The fixture with no unknown hiragana nodes, a 2x3 matrix and two words at the i16 extremes:
    あ = (left 1, right 1, 32767), い = (left 2, right 1, -32768).  get(r, l) = data[2 l + r]:
    BOS -> あ data[2] = 0; あ -> あ data[3] = 32767; あ / い -> い data[5] = -32768; あ / い -> EOS data[1] = 0."""
    p = fixture_dict_parts()
    p["invoke_list"] = np.array([0, 1, 0], dtype=np.uint8)
    p["group_list"] = np.array([0, 1, 0], dtype=np.uint8)
    p["sorted_keywords"] = [A, I]
    p["morphs"] = [[1, 1, 32767], [2, 1, -32768]]
    p["conn_rows"], p["conn_cols"], p["conn_data"] = 2, 3, [0, 0, 0, 32767, 0, -32768]
    return p


def transposed_parts():
    """A 3x2 matrix (rows > cols) where the layout decides the token: あ has two records, (1, 0) = id 1 and (1, 2) = id 2,
    い = (1, 0) = id 3.  get(r, l) = data[3 l + r]: id 1 -> い reads data[3] = 0, id 2 -> い reads data[5] = -100, so id 2
    wins.  Indexed by cols instead (data[2 l + r]) the two read data[2] = -500 and data[4] = 0 and id 1 would win."""
    p = fixture_dict_parts()
    p["invoke_list"] = np.array([0, 1, 0], dtype=np.uint8)
    p["sorted_keywords"] = [A, A, I]
    p["morphs"] = [[1, 0, 0], [1, 2, 0], [1, 0, 0]]
    p["conn_rows"], p["conn_cols"], p["conn_data"] = 3, 2, [0, 0, -500, 0, 0, -100]
    return p


# ------------------------------------------------------------------------------------------------------------------------------------ lattices
def lattice_from_pyref(pd, text):
    """oracle/pyref.lattice -> kanpyo_amd.lattice.Lattice (tests/test_lattice_cpu.py; the device dump is compared with it in the gpu tests)."""
    from kanpyo_amd.lattice import Lattice, Node
    from kanpyo_amd.token import TokenClass
    from oracle import pyref

    raw = text.encode("utf-8")
    nodes, edges, dp, pre = pyref.lattice(pd, text)
    out = []
    for i, (cls, nid, bpos, cpos, morph, bl, cl) in enumerate(nodes):
        out.append(Node(nid, TokenClass(cls), bpos, cpos, cpos + cl, morph[0], morph[1], morph[2], raw[bpos : bpos + bl].decode("utf-8"),
                        0 if dp[i] is None else dp[i], pre[i]))
    return Lattice(out, [list(e) for e in edges])


# ---------------------------------------------------------------------------------------------------------------------------- MeCab-format sources
CHAR_DEF = """# test char.def in MeCab format
DEFAULT         0 1 0  # mandatory
SPACE           0 1 0
KANJI           0 0 2
HIRAGANA        0 1 2
KATAKANA        1 1 2
NUMERIC         1 1 0

0x0020 SPACE
0x0030..0x0039 NUMERIC
0x3041..0x309F  HIRAGANA
0x30A1..0x30FF  KATAKANA
0x4E00..0x9FA5  KANJI
0x4E00 NUMERIC KANJI  # first category wins (char_def.rs:65-71)
"""
UNK_DEF = "DEFAULT,5,5,4769,記号,一般,*,*,*,*,*\nKATAKANA,1,1,3000,名詞,一般,*,*,*,*,*\nKATAKANA,1,1,2500,名詞,固有,*,*,*,*,*\nHIRAGANA,2,2,9000,助詞,*,*,*,*,*,*\nKANJI,1,1,8000,名詞,一般,*,*,*,*,*\nNUMERIC,3,3,1000,名詞,数,*,*,*,*,*\nSPACE,4,4,100,記号,空白,*,*,*,*,*\n"
LEX_A = "東京,1,1,3000,名詞,固有名詞,地域,一般,*,*,東京,トウキョウ,トーキョー\n東京都,1,1,3500,名詞,固有名詞,地域,一般,*,*,東京都,トウキョウト,トーキョート\nに,2,2,500,助詞,格助詞,一般,*,*,*,に,ニ,ニ\n"
LEX_B = "住む,6,6,4000,動詞,自立,*,*,五段・マ行,基本形,住む,スム,スム\nに,2,2,700,助詞,副助詞,*,*,*,*,に,ニ,ニ\n都,1,1,6000,名詞,接尾,地域,*,*,*,都,ト,ト\n\"a,b\",1,1,100,名詞,一般,*,*,*,*,\"a,b\",*,*\n"


def mecab_matrix(n=7):
    lines = [f"{n} {n}"]
    for r in range(n):
        for c in range(n):
            lines.append(f"{r} {c} {(r * 31 + c * 17) % 200 - 100}")
    return "\n".join(lines) + "\n"
