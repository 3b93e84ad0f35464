"""The layout of tests/ itself, from its source text: helpers live in helper modules (kernel_cases, kernel_run, <topic>_cases, <topic>_ref), so that
no test module is imported by another module -- an import-time change in a GPU test cannot break the CPU suite -- and the `libs` fixture exists once."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = {os.path.basename(p): open(p, encoding="utf-8").read() for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def test_no_module_imports_a_test_module():
    found = [(name, m.group(0).strip()) for name, text in SOURCES.items()
             for m in re.finditer(r"^[ \t]*(?:from[ \t]+test_\w+[ \t]+import\b|import[ \t]+test_\w+).*$", text, re.M)]
    assert not found, found


def test_the_libs_fixture_is_defined_once():
    assert [name for name, text in SOURCES.items() if re.search(r"^[ \t]*def libs\b", text, re.M)] == ["kernel_run.py"]
