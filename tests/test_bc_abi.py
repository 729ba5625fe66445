"""CPU checks of betweenness centrality's place in the product boundary: the header declares
grx_bc, the library exports it and the Python layer offers essentials_amd.bc."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def test_header_declares_grx_bc():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_bc\s*\(", text)


def test_library_exports_grx_bc():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_bc")


def test_python_layer_offers_bc():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.bc) and "bc" in ea.__all__
    assert "grx_bc" in _SIGNATURES
