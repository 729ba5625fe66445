"""CPU checks of connected components' place in the product boundary (the header declares grx_cc,
the library exports it, the Python layer offers essentials_amd.cc) and of the numpy oracle the GPU
tests compare against (tests/cc_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cc_oracle import KNOWN, components, csr, known_csr, mtx_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_cc\s*\(", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_cc")


def test_python_layer_offers_cc():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.cc) and "cc" in ea.__all__
    assert "grx_cc" in _SIGNATURES


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, want = known_csr(name)
    labels, count = components(ap, aj)
    assert labels.dtype == np.int32 and labels.tolist() == want.tolist()
    assert count == len(set(want.tolist()))


def _random_multigraph(seed=4, n=300, m=260):
    """Symmetric CSR with repeated edges, self loops and shuffled rows; several components."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def _random_directed(seed=11, n=400, m=330):
    rng = np.random.default_rng(seed)
    return csr(n, rng.integers(0, n, size=(m, 2)), symmetric=False)


def _transpose(ap, aj):
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    return csr(n, np.stack([np.asarray(aj, np.int64), src], 1), symmetric=False)


def _min_labels(n, membership):
    """Arbitrary component numbers -> the smallest vertex id of each component."""
    membership = np.asarray(membership)
    smallest = np.full(int(membership.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(smallest, membership, np.arange(n))
    return smallest[membership]


GRAPHS = {"chesapeake": lambda: mtx_csr(CHESAPEAKE), "multigraph": _random_multigraph, "directed": _random_directed}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_oracle_matches_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    ap, aj = GRAPHS[name]()
    n = len(ap) - 1
    m = sp.csr_matrix((np.ones(len(aj), np.int8), aj, ap), shape=(n, n))
    count, membership = connected_components(m, directed=True, connection="weak")
    labels, got = components(ap, aj)
    assert got == count and labels.tolist() == _min_labels(n, membership).tolist()
    assert count == 1 if name == "chesapeake" else count > 5


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_oracle_matches_networkx(name):
    nx = pytest.importorskip("networkx")
    ap, aj = GRAPHS[name]()
    n = len(ap) - 1
    G = nx.Graph()
    G.add_nodes_from(range(n))
    src = np.repeat(np.arange(n), np.diff(ap))
    G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
    want = np.empty(n, np.int64)
    parts = list(nx.connected_components(G))
    for part in parts:
        want[list(part)] = min(part)
    labels, got = components(ap, aj)
    assert got == len(parts) and labels.tolist() == want.tolist()


def test_oracle_ignores_row_order_and_direction():
    ap, aj = _random_directed()
    want = components(ap, aj)
    rng = np.random.default_rng(1)
    shuffled = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(shuffled[ap[u]:ap[u + 1]])
    got = components(ap, shuffled)
    assert (got[0] == want[0]).all() and got[1] == want[1]
    got = components(*_transpose(ap, aj))
    assert (got[0] == want[0]).all() and got[1] == want[1]
    assert want[1] > 5 and (want[0] <= np.arange(len(ap) - 1)).all()


def test_oracle_on_a_shuffled_path():
    """Labels travel far: a path of 20 001 vertices under a random numbering is one component."""
    n = 20001
    order = np.random.default_rng(2).permutation(n)
    ap, aj = csr(n, np.stack([order[:-1], order[1:]], 1))
    labels, count = components(ap, aj)
    assert count == 1 and not labels.any()
