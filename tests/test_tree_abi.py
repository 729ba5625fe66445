"""CPU checks of the shortest-path trees' place in the product boundary (the header declares
grx_bfs_predecessors and grx_sssp_predecessors, the library exports them, the Python layer offers
essentials_amd.predecessors and .path) and of the oracle the GPU tests compare against
(tests/tree_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tree_oracle import FLT_UNREACHED, INT_UNREACHED, chain_steps, csr, doubling_rounds, tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def test_header_declares_both_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_bfs_predecessors\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*int32_t\s+source,"
                     r"\s*const\s+int32_t\s*\*\s*d_depths,\s*int32_t\s*\*\s*d_predecessors,"
                     r"\s*int64_t\s*\*\s*h_orphans,\s*int64_t\s*\*\s*h_violations,"
                     r"\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)
    assert re.search(r"\bint\s+grx_sssp_predecessors\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*int32_t\s+source,"
                     r"\s*const\s+float\s*\*\s*d_distances,\s*int32_t\s*\*\s*d_predecessors,\s*int32_t\s*\*\s*d_hops,"
                     r"\s*int64_t\s*\*\s*h_orphans,\s*int64_t\s*\*\s*h_violations,"
                     r"\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", text)


def test_the_traversals_name_the_new_calls():
    text = open(HEADER).read()
    for call in ("grx_bfs", "grx_sssp"):
        comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + call + r"\s*\(", text, flags=re.S).group(1)
        assert call + "_predecessors" in comment


def test_library_exports_both_calls():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_bfs_predecessors") and hasattr(lib, "grx_sssp_predecessors")


def test_python_layer_offers_predecessors_and_path():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.predecessors) and callable(ea.path)
    assert "predecessors" in ea.__all__ and "path" in ea.__all__
    assert "grx_bfs_predecessors" in _SIGNATURES and "grx_sssp_predecessors" in _SIGNATURES
    assert len(_SIGNATURES["grx_bfs_predecessors"][1]) == 9 and len(_SIGNATURES["grx_sssp_predecessors"][1]) == 10


# ---- the oracle gives the hand values ------------------------------------------------------------------

def test_four_cycle():
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3), (3, 0)])
    got = tree(ap, aj, aw, np.array([0, 1, 2, 1], np.int32), 0)
    assert got["pred"].tolist() == [0, 0, 1, 0] and got["hops"].tolist() == [0, 1, 2, 1]  # 2: parents 1 and 3
    assert (got["orphans"], got["violations"], got["reached"]) == (0, 0, 4)
    got = tree(ap, aj, aw, np.array([0, 1, 2, 1], np.float32), 0)
    assert got["pred"].tolist() == [0, 0, 1, 0] and got["hops"].tolist() == [0, 1, 2, 1]


def test_diamond_picks_the_smaller_of_two_equal_parents():
    # 0 -> {2, 1} -> 3, the larger parent listed first in every row
    ap, aj, aw = csr(4, [(0, 2), (0, 1), (2, 3), (1, 3)], weights=[2.0, 1.0, 1.0, 2.0], symmetric=False)
    assert tree(ap, aj, aw, np.array([0, 1, 2, 3], np.float32), 0)["pred"].tolist() == [0, 0, 0, 1]
    assert tree(ap, aj, aw, np.array([0, 1, 1, 2], np.int32), 0)["pred"].tolist() == [0, 0, 0, 1]
    assert tree(ap, aj, aw, np.array([0, 1, 2, 3], np.float32), 0)["violations"] == 0
    # with the way through 2 the lighter one, 3 has one parent
    ap, aj, aw = csr(4, [(0, 2), (0, 1), (2, 3), (1, 3)], weights=[1.0, 1.0, 1.0, 2.0], symmetric=False)
    assert tree(ap, aj, aw, np.array([0, 1, 1, 2], np.float32), 0)["pred"].tolist() == [0, 0, 0, 2]


def test_zero_and_absorbed_weights_make_an_orphan():
    for light in (0.0, 2.0 ** -30):
        ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)], weights=[1.0, light, 1.0], symmetric=False)
        got = tree(ap, aj, aw, np.array([0, 1, 1, 2], np.float32), 0)
        assert got["pred"].tolist() == [0, 0, -2, 2] and got["hops"].tolist() == [0, 1, -1, -1]
        assert (got["orphans"], got["violations"], got["reached"]) == (1, 0, 4)
        assert doubling_rounds(got["pred"]) == 0  # the longest chain is one step: 1 -> 0 and 3 -> 2


def test_violations_and_unreached():
    ap, aj, aw = csr(5, [(0, 1), (1, 2), (2, 3)], symmetric=False)
    depths = np.array([0, 1, 4, INT_UNREACHED, INT_UNREACHED], np.int32)
    got = tree(ap, aj, aw, depths, 0)
    # 1 -> 2 violates (2 < 4) and 2 -> 3 violates (5 < unreached); 2 has no parent, 3 and 4 are unreached
    assert got["pred"].tolist() == [0, 0, -2, -1, -1] and got["hops"].tolist() == [0, 1, -1, -1, -1]
    assert (got["orphans"], got["violations"], got["reached"]) == (1, 2, 3)
    dist = np.array([0, 1, np.nan, FLT_UNREACHED, FLT_UNREACHED], np.float32)
    got = tree(ap, aj, aw, dist, 0)  # a NaN qualifies nothing and violates nothing, and counts as reached
    assert got["pred"].tolist() == [0, 0, -2, -1, -1] and (got["orphans"], got["violations"]) == (1, 0)
    assert got["reached"] == 3


def test_chains_and_rounds():
    pred = np.array([0, 0, 1, 2, 3, -1, -2, 6, 7])
    steps, end = chain_steps(pred)
    assert steps.tolist() == [0, 1, 2, 3, 4, 0, 0, 1, 2] and end.tolist() == [0, 0, 0, 0, 0, 5, 6, 6, 6]
    assert doubling_rounds(pred) == 2
    assert [doubling_rounds(np.concatenate([[0], np.arange(L)])) for L in (1, 2, 3, 4, 5, 8, 9)] == [0, 1, 2, 2, 3, 3, 4]
    assert doubling_rounds(np.array([0])) == 0 and doubling_rounds(np.zeros(0, np.int64)) == 0
    assert doubling_rounds(np.concatenate([[0], np.arange(4999)])) == 13


def test_path_on_hand_arrays():
    import essentials_amd as ea
    import tree_oracle
    pred = np.array([2, -1, 2, 0, 3, -2, 5], np.int32)  # source 2; 1 unreached; 5 an orphan with 6 behind it
    for walk in (ea.path, tree_oracle.path):
        assert walk(pred, 4) == [2, 0, 3, 4]
        assert walk(pred, 2) == [2]
        assert walk(pred, 1) == [] and walk(pred, 5) == [] and walk(pred, 6) == []
    assert ea.path(pred, 7) == [] and ea.path(pred, -1) == []
    assert ea.path(np.array([1, 0], np.int32), 0) == []  # a cycle ends after V steps
    torch = pytest.importorskip("torch")
    assert ea.path(torch.from_numpy(pred), 4) == [2, 0, 3, 4]
