"""Every function include/quartetscores_hip.h declares is defined by the built library (no GPU): the C-ABI layer is spread over several
files, and a function lost between them would otherwise show only where something calls it."""
import ctypes
import os
import re

from quartetscores_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "quartetscores_hip.h")


def declared_functions():
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # comments name functions too ("see qs_sync()")
    text = re.sub(r"//[^\n]*", " ", text)
    return sorted(set(re.findall(r"\b(qs_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_function_is_exported():
    names = declared_functions()
    assert len(names) >= 64, names            # the header of the commit this test came with declares 64
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_the_binding_lists_what_the_header_declares():
    assert sorted(_lib.EXPORTS) == declared_functions()
