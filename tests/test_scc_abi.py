"""CPU checks of strongly connected components' place in the product boundary (the header declares
grx_scc, the library exports it, the Python layer offers essentials_amd.scc) and of the oracle the
GPU tests compare against (tests/scc_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cc_oracle
from scc_oracle import KNOWN, csr, known_csr, mtx_csr, strong_components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_scc\s*\(", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_scc")


def test_python_layer_offers_scc():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.scc) and "scc" in ea.__all__
    assert "grx_scc" in _SIGNATURES


def test_known_has_the_cases():
    assert len(KNOWN) >= 18 and sum(both for _, _, both, _ in KNOWN.values()) == 3


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, want = known_csr(name)
    labels, count = strong_components(ap, aj)
    assert labels.dtype == np.int32 and labels.tolist() == want.tolist()
    assert count == len(set(want.tolist()))


def _random_directed(seed=11, n=400, m=600):
    rng = np.random.default_rng(seed)
    return csr(n, rng.integers(0, n, size=(m, 2)), symmetric=False)


def _chain_of_two_cycles(count=300):
    a = 2 * np.arange(count, dtype=np.int64)
    e = np.concatenate([np.stack([a, a + 1], 1), np.stack([a + 1, a], 1), np.stack([a[:-1] + 1, a[1:]], 1)])
    return csr(2 * count, e, symmetric=False)


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


GRAPHS = {"chesapeake": lambda: mtx_csr(CHESAPEAKE), "directed": _random_directed, "two_cycles": _chain_of_two_cycles}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_oracle_matches_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    ap, aj = GRAPHS[name]()
    n = len(ap) - 1
    m = sp.csr_matrix((np.ones(len(aj), np.int8), aj, ap), shape=(n, n))
    count, membership = connected_components(m, directed=True, connection="strong")
    labels, got = strong_components(ap, aj)
    assert got == count and labels.tolist() == _min_labels(n, membership).tolist()
    if name == "chesapeake":
        assert count == 1
    if name == "two_cycles":
        assert count == 300 and labels.tolist() == (np.arange(n) // 2 * 2).tolist()
    if name == "directed":
        assert 5 < count < n  # singletons and at least one component with a cycle


def test_oracle_ignores_row_order_and_transposing():
    ap, aj = _random_directed()
    want = strong_components(ap, aj)
    rng = np.random.default_rng(1)
    shuffled = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(shuffled[ap[u]:ap[u + 1]])
    got = strong_components(ap, shuffled)
    assert (got[0] == want[0]).all() and got[1] == want[1]
    got = strong_components(*_transpose(ap, aj))
    assert (got[0] == want[0]).all() and got[1] == want[1]


def test_oracle_is_the_weak_one_on_a_symmetric_csr():
    rng = np.random.default_rng(4)
    ap, aj = csr(300, rng.integers(0, 300, size=(260, 2)))
    want = cc_oracle.components(ap, aj)
    got = strong_components(ap, aj)
    assert (got[0] == want[0]).all() and got[1] == want[1] and got[1] > 5


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_labels_are_representatives(name):
    ap, aj = GRAPHS[name]()
    labels, count = strong_components(ap, aj)
    ids = np.arange(len(ap) - 1)
    assert (labels <= ids).all() and (labels[labels] == labels).all()
    assert count == int((labels == ids).sum())
