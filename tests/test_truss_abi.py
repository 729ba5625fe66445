"""CPU checks of k-truss decomposition's place in the product boundary (the header declares
grx_truss, the library exports it, the Python layer offers essentials_amd.truss) and of the oracle
the GPU tests compare against (tests/truss_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from truss_oracle import KNOWN, csr, known_csr, mtx_csr, simple_csr, truss_numbers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares_grx_truss():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_truss\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*int32_t\s*\*\s*d_truss,"
                     r"\s*int32_t\s*\*\s*h_max_truss,\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)",
                     text)


def test_library_exports_grx_truss():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_truss")


def test_python_layer_offers_truss():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.truss) and "truss" in ea.__all__
    assert "grx_truss" in _SIGNATURES


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, want = known_csr(name)
    values, largest, levels = truss_numbers(ap, aj)
    assert values.dtype == np.int32 and values.tolist() == want.tolist()
    assert largest == (int(want.max()) if len(want) else 0)
    assert levels == len(set(want.tolist()))


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def _networkx_truss(nx, ap, aj):
    """Trussness per entry by repeated nx.k_truss: an edge of the k-truss has at least k."""
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
    of = {}
    k = 2
    while True:
        T = nx.k_truss(G, k)
        if T.number_of_edges() == 0:
            break
        for a, b in T.edges():
            of[(a, b)] = of[(b, a)] = k
        k += 1
    return np.asarray([of[(int(a), int(b))] for a, b in zip(src, aj)], np.int32), G.number_of_edges()


@pytest.mark.parametrize("which,edges,values", [("chesapeake", 170, {2, 3, 4, 5}), ("multigraph", 345, {2, 3, 4})])
def test_oracle_matches_networkx(which, edges, values):
    nx = pytest.importorskip("networkx")
    ap, aj = mtx_csr(CHESAPEAKE) if which == "chesapeake" else simple_csr(*_random_multigraph())
    want, m = _networkx_truss(nx, ap, aj)
    got, largest, levels = truss_numbers(ap, aj)
    assert m == edges and len(aj) == 2 * edges
    assert got.tolist() == want.tolist()
    assert set(got.tolist()) == values and largest == max(values) and levels == len(values)


def test_oracle_ignores_row_order_repeats_and_loops():
    ap, aj = _random_multigraph()
    n = len(ap) - 1
    sap, saj = simple_csr(ap, aj)
    simple = truss_numbers(sap, saj)
    of = {}
    for u in range(n):
        for v, t in zip(saj[sap[u]:sap[u + 1]], simple[0][sap[u]:sap[u + 1]]):
            of[(u, int(v))] = int(t)
    got = truss_numbers(ap, aj)
    src = np.repeat(np.arange(n), np.diff(ap))
    assert (src == aj).any() and len(aj) > len(saj)
    assert got[0].tolist() == [0 if u == v else of[(int(u), int(v))] for u, v in zip(src, aj)]
    assert got[1:] == simple[1:]
