"""CPU checks of the minimum spanning forest's place in the product boundary (the header declares
grx_mst, the library exports it, the Python layer offers essentials_amd.mst) and of the numpy oracle
the GPU tests compare against (tests/mst_oracle.py): its vectorised Boruvka against the definition
(Kruskal on the 64-bit keys), hand-written answers, scipy and networkx."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cc_oracle import components
from mst_oracle import KNOWN, forest, known_csr, kruskal, mtx_csr, ordered_bits, weighted_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_mst\s*\(", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_mst")


def test_python_layer_offers_mst():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.mst) and "mst" in ea.__all__
    assert "grx_mst" in _SIGNATURES


def test_ordered_bits_is_monotone():
    values = np.array([-np.inf, -3.5, -1.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.0, 64.0, np.inf], np.float32)
    bits = ordered_bits(values).astype(np.int64)
    assert (np.diff(bits) > 0).all()


def same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1] == b[1] and a[2].tolist() == b[2].tolist()


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, ax, entries, weight = known_csr(name)
    labels = components(ap, aj)[0]
    for got in (forest(ap, aj, ax), kruskal(ap, aj, ax)):
        assert got[0].dtype == np.int32 and got[0].tolist() == entries.tolist()
        assert got[1] == weight
        assert got[2].dtype == np.int32 and got[2].tolist() == labels.tolist()
        assert len(got[0]) == len(labels) - len(set(labels.tolist()))


def _chesapeake():
    ap, aj = mtx_csr(CHESAPEAKE)
    return ap, aj, np.ones(len(aj), np.float32)


def _random_multigraph(seed=4, n=300, m=260):
    """Symmetric CSR with repeated edges, self loops, shuffled rows and weights from {1..4};
    several components."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj, ax = weighted_csr(n, e, rng.integers(1, 5, len(e)))
    for u in range(n):
        order = rng.permutation(ap[u + 1] - ap[u]) + ap[u]
        aj[ap[u]:ap[u + 1]], ax[ap[u]:ap[u + 1]] = aj[order], ax[order]
    return ap, aj, ax


def _random_directed(seed=11, n=400, m=330):
    rng = np.random.default_rng(seed)
    return weighted_csr(n, rng.integers(0, n, size=(m, 2)), rng.integers(1, 5, m), symmetric=False)


GRAPHS = {"chesapeake": _chesapeake, "multigraph": _random_multigraph, "directed": _random_directed}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forest_is_kruskal(name):
    ap, aj, ax = GRAPHS[name]()
    a, b = forest(ap, aj, ax), kruskal(ap, aj, ax)
    assert same(a, b)
    labels, count = components(ap, aj)
    assert a[2].tolist() == labels.tolist() and len(a[0]) == len(ap) - 1 - count
    src = np.repeat(np.arange(len(ap) - 1), np.diff(ap))
    assert (src[a[0]] != aj[a[0]]).all() and (np.diff(a[0]) > 0).all()
    assert count == 1 if name == "chesapeake" else count > 5


def _lightest_of_parallel(ap, aj, ax):
    """Undirected simple graph: (a < b, the smallest weight among the entries that join them)."""
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    dst = np.asarray(aj, np.int64)
    keep = src != dst
    a, b, w = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep], np.asarray(ax, np.float64)[keep]
    pair, inverse = np.unique(a * n + b, return_inverse=True)
    low = np.full(len(pair), np.inf)
    np.minimum.at(low, inverse, w)
    return n, pair // n, pair % n, low


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_weight_matches_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import minimum_spanning_tree
    ap, aj, ax = GRAPHS[name]()
    n, a, b, w = _lightest_of_parallel(ap, aj, ax)
    tree = minimum_spanning_tree(sp.csr_matrix((w, (a, b)), shape=(n, n)))
    got = forest(ap, aj, ax)
    assert got[1] == float(tree.sum()) and len(got[0]) == tree.nnz


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_weight_matches_networkx(name):
    nx = pytest.importorskip("networkx")
    ap, aj, ax = GRAPHS[name]()
    n, a, b, w = _lightest_of_parallel(ap, aj, ax)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from((int(x), int(y), float(z)) for x, y, z in zip(a, b, w))
    tree = nx.minimum_spanning_tree(G)
    got = forest(ap, aj, ax)
    assert got[1] == float(sum(d["weight"] for _, _, d in tree.edges(data=True)))
    assert len(got[0]) == tree.number_of_edges()


def test_weight_ignores_row_order_and_direction():
    ap, aj, ax = _random_directed()
    want = forest(ap, aj, ax)
    rng = np.random.default_rng(1)
    sj, sx = aj.copy(), ax.copy()
    for u in range(len(ap) - 1):
        order = rng.permutation(ap[u + 1] - ap[u]) + ap[u]
        sj[ap[u]:ap[u + 1]], sx[ap[u]:ap[u + 1]] = aj[order], ax[order]
    got = forest(ap, sj, sx)
    assert got[1] == want[1] and len(got[0]) == len(want[0]) and got[2].tolist() == want[2].tolist()
    assert same(got, kruskal(ap, sj, sx))
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    tp, tj, tx = weighted_csr(n, np.stack([np.asarray(aj, np.int64), src], 1), ax, symmetric=False)
    got = forest(tp, tj, tx)
    assert got[1] == want[1] and len(got[0]) == len(want[0]) and got[2].tolist() == want[2].tolist()
    assert len(want[0]) > 100


def test_oracle_on_a_shuffled_path():
    """Hooks travel far: a path of 20 001 vertices under a random numbering, every weight equal,
    keeps all its V - 1 edges, one stored direction of each."""
    n = 20001
    order = np.random.default_rng(2).permutation(n)
    ap, aj, ax = weighted_csr(n, np.stack([order[:-1], order[1:]], 1), np.ones(n - 1))
    entries, weight, labels = forest(ap, aj, ax)
    assert len(entries) == n - 1 and weight == float(n - 1) and not labels.any()
    src = np.repeat(np.arange(n), np.diff(ap))
    a, b = np.minimum(src[entries], aj[entries]), np.maximum(src[entries], aj[entries])
    assert len(np.unique(a.astype(np.int64) * n + b)) == n - 1
