"""CPU checks of triangle counting's place in the product boundary (the header declares grx_tc,
the library exports it, the Python layer offers essentials_amd.tc) and of the numpy oracle the
GPU tests compare against (tests/tc_oracle.py)."""
import ctypes as C
import os
import re
from math import comb

import numpy as np
import pytest

from tc_oracle import KNOWN, KNOWN_COUNTS, KNOWN_T, csr, mtx_csr, triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def test_header_declares_grx_tc():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_tc\s*\(", text)


def test_library_exports_grx_tc():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_tc")


def test_python_layer_offers_tc():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.tc) and "tc" in ea.__all__
    assert "grx_tc" in _SIGNATURES


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj = KNOWN[name]
    counts, t = triangles(np.array(ap), np.array(aj))
    assert counts.tolist() == KNOWN_COUNTS and t == KNOWN_T


@pytest.mark.parametrize("n", [3, 4, 7, 12])
def test_oracle_complete_graph(n):
    ap, aj = csr(n, [(a, b) for a in range(n) for b in range(a + 1, n)])
    counts, t = triangles(ap, aj)
    assert (counts == comb(n - 1, 2)).all() and t == comb(n, 3)


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def test_oracle_matches_networkx():
    nx = pytest.importorskip("networkx")
    for ap, aj in (mtx_csr(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")), _random_multigraph()):
        n = len(ap) - 1
        G = nx.Graph()
        G.add_nodes_from(range(n))
        src = np.repeat(np.arange(n), np.diff(ap))
        G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj) if a != b)
        want = nx.triangles(G)
        counts, t = triangles(ap, aj)
        assert counts.tolist() == [want[v] for v in range(n)]
        assert 3 * t == sum(want.values()) and t > 0
