"""CPU checks of k-core decomposition's place in the product boundary (the header declares
grx_kcore and grx_graph_simple, the library exports them, the Python layer offers
essentials_amd.kcore and Graph.simple) and of the numpy oracle the GPU tests compare against
(tests/kcore_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kcore_oracle import KNOWN, core_numbers, csr, known_csr, mtx_csr, simple_csr, write_mtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


@pytest.mark.parametrize("name", ["grx_kcore", "grx_graph_simple"])
def test_header_declares(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, text)


@pytest.mark.parametrize("name", ["grx_kcore", "grx_graph_simple"])
def test_library_exports(name):
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, name)


def test_python_layer_offers_kcore():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.kcore) and "kcore" in ea.__all__
    assert callable(ea.Graph.simple)
    assert "grx_kcore" in _SIGNATURES and "grx_graph_simple" in _SIGNATURES


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, want = known_csr(name)
    core, degeneracy, levels = core_numbers(ap, aj)
    assert core.dtype == np.int32 and core.tolist() == want.tolist()
    assert degeneracy == (int(want.max()) if len(want) else 0)
    assert levels == len(set(want[want > 0].tolist()))


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
    for ap, aj in (mtx_csr(CHESAPEAKE), simple_csr(*_random_multigraph())):
        n = len(ap) - 1
        G = nx.Graph()
        G.add_nodes_from(range(n))
        src = np.repeat(np.arange(n), np.diff(ap))
        G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
        want = nx.core_number(G)
        core, degeneracy, _ = core_numbers(ap, aj)
        assert core.tolist() == [want[v] for v in range(n)]
        assert degeneracy == max(want.values()) > 1


def test_oracle_counts_every_entry():
    """A multigraph's core numbers are not its simple graph's: repeats and self loops count."""
    ap, aj = _random_multigraph()
    multi = core_numbers(ap, aj)[0]
    simple = core_numbers(*simple_csr(ap, aj))[0]
    assert (multi >= simple).all() and (multi > simple).any()


def test_oracle_ignores_row_order():
    ap, aj = _random_multigraph(seed=9)
    want = core_numbers(ap, aj)
    rng = np.random.default_rng(1)
    aj = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    got = core_numbers(ap, aj)
    assert (got[0] == want[0]).all() and got[1:] == want[1:]


def test_simple_csr_and_write_mtx(tmp_path):
    ap, aj = _random_multigraph()
    ax = np.random.default_rng(3).integers(1, 64, len(aj)).astype(np.float32)
    sap, saj, sax = simple_csr(ap, aj, ax)
    n = len(ap) - 1
    for u in range(n):
        row, w = aj[ap[u]:ap[u + 1]], ax[ap[u]:ap[u + 1]]
        cols = sorted(set(row.tolist()) - {u})
        assert saj[sap[u]:sap[u + 1]].tolist() == cols
        assert sax[sap[u]:sap[u + 1]].tolist() == [float(w[row == c].min()) for c in cols]
    # the file holds each undirected edge once and loads back as the same CSR
    path = str(tmp_path / "simple.mtx")
    write_mtx(path, sap, saj)
    bap, baj = mtx_csr(path)
    assert (bap == sap).all() and (baj == saj).all()
