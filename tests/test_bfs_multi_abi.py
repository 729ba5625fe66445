"""CPU checks of multi-source BFS's place in the product boundary (the header declares
grx_bfs_multi, the library exports it, the Python layer offers essentials_amd.bfs_multi) and of the
oracle the GPU tests compare against (tests/bfs_multi_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bfs_multi_oracle import UNREACHED, csr, mtx_csr, multi_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares_grx_bfs_multi():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_bfs_multi\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,"
                     r"\s*const\s+int32_t\s*\*\s*h_sources,\s*int32_t\s+n_sources,\s*int32_t\s*\*\s*d_depths,"
                     r"\s*int64_t\s*\*\s*h_reached,\s*int64_t\s*\*\s*h_depth_sum,\s*int32_t\s*\*\s*h_eccentricity,"
                     r"\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)


def test_library_exports_grx_bfs_multi():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_bfs_multi")


def test_python_layer_offers_bfs_multi():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.bfs_multi) and "bfs_multi" in ea.__all__
    assert "grx_bfs_multi" in _SIGNATURES


@pytest.mark.parametrize("n", [1, 2, 7, 64, 65])
def test_oracle_on_a_path(n):
    v = np.arange(n - 1)
    ap, aj = csr(n, np.stack([v, v + 1], 1))
    got = multi_source(ap, aj, [0, n - 1, n // 2])
    assert got["depths"].dtype == np.int32 and got["depths"][0].tolist() == list(range(n))
    assert got["depths"][1].tolist() == list(range(n))[::-1]
    assert got["eccentricity"].tolist() == [n - 1, n - 1, max(n // 2, n - 1 - n // 2)]
    assert got["depth_sum"][0] == n * (n - 1) // 2 and got["reached"].tolist() == [n] * 3
    assert got["levels"] == [n] and len(got["active"]) == n
    assert got["active"][0] == len({0, n - 1, n // 2})


def test_oracle_on_a_star():
    leaves = 9
    ap, aj = csr(leaves + 1, np.stack([np.zeros(leaves, int), np.arange(1, leaves + 1)], 1))
    got = multi_source(ap, aj, [0, 3, 3])
    assert got["depths"][0].tolist() == [0] + [1] * leaves
    assert got["depths"][1].tolist() == [1, 2, 2, 0] + [2] * (leaves - 3)
    assert (got["depths"][2] == got["depths"][1]).all()
    assert got["eccentricity"].tolist() == [1, 2, 2]
    assert got["depth_sum"].tolist() == [leaves, 1 + 2 * (leaves - 1)] + [1 + 2 * (leaves - 1)]
    assert got["reached"].tolist() == [leaves + 1] * 3
    # level 0: hub and leaf 3; level 1: hub (for the leaf) and all leaves (for the hub); level 2: the other leaves
    assert got["levels"] == [3] and got["active"] == [2, leaves + 1, leaves - 1]
    assert got["traversed"] == (leaves + 1) + (leaves + leaves) + (leaves - 1)


def test_oracle_on_two_triangles():
    ap, aj = csr(7, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)])
    got = multi_source(ap, aj)  # every vertex; vertex 6 is isolated
    assert got["depths"].shape == (7, 7)
    assert got["depths"][0].tolist() == [0, 1, 1] + [UNREACHED] * 4
    assert got["depths"][4].tolist() == [UNREACHED] * 3 + [1, 0, 1, UNREACHED]
    assert got["depths"][6].tolist() == [UNREACHED] * 6 + [0]
    assert got["reached"].tolist() == [3] * 6 + [1]
    assert got["depth_sum"].tolist() == [2] * 6 + [0]
    assert got["eccentricity"].tolist() == [1] * 6 + [0]
    assert got["levels"] == [2] and got["active"] == [7, 6]


def test_oracle_counts_levels_per_batch_of_64():
    n = 70
    v = np.arange(n - 1)
    ap, aj = csr(n, np.stack([v, v + 1], 1))
    got = multi_source(ap, aj)
    # the first batch holds vertex 0 (eccentricity 69), the second 64..69 (the largest: 69 again)
    assert got["levels"] == [70, 70] and got["eccentricity"][35] == 35
    directed = csr(n, np.stack([v, v + 1], 1), symmetric=False)
    got = multi_source(*directed)
    assert got["levels"] == [70, 6] and got["reached"].tolist() == list(range(n, 0, -1))


def test_oracle_matches_networkx():
    nx = pytest.importorskip("networkx")
    ap, aj = mtx_csr(CHESAPEAKE)
    n = len(ap) - 1
    assert n == 39 and len(aj) == 340
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((u, int(w)) for u in range(n) for w in aj[ap[u]:ap[u + 1]])
    got = multi_source(ap, aj)
    for s in range(n):
        want = nx.single_source_shortest_path_length(G, s)
        row = [want.get(w, UNREACHED) for w in range(n)]
        assert got["depths"][s].tolist() == row
        assert got["reached"][s] == len(want) and got["depth_sum"][s] == sum(want.values())
        assert got["eccentricity"][s] == max(want.values())
