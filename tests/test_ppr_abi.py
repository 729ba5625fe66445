"""CPU checks of batched personalized PageRank's place in the product boundary (the header declares
grx_ppr, the library exports it, the Python layer offers essentials_amd.ppr) and of the oracle the
GPU tests compare against (tests/ppr_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bfs_multi_oracle import mtx_csr
from ppr_oracle import csr, exact_cases, exact_in_float32, ppr, rounding_bound, transpose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares_grx_ppr():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_ppr\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,"
                     r"\s*const\s+int32_t\s*\*\s*h_seeds,\s*int32_t\s+n_seeds,\s*float\s+alpha,\s*float\s+tol,"
                     r"\s*float\s*\*\s*d_p,\s*int32_t\s*\*\s*h_iterations,\s*float\s*\*\s*h_residual,"
                     r"\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)


def test_library_exports_grx_ppr():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_ppr")


def test_python_layer_offers_ppr():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.ppr) and "ppr" in ea.__all__
    assert "grx_ppr" in _SIGNATURES


def test_oracle_on_a_two_cycle():
    ap, aj, aw = csr(2, [(0, 1)])
    got = ppr(ap, aj, aw, [0, 1], alpha=0.5, tol=0, max_iterations=3)
    # p1 = (1/2, 1/2), p2 = (3/4, 1/4), p3 = (5/8, 3/8): the fixed point is (2/3, 1/3)
    assert got["p"][0].tolist() == [0.625, 0.375] and got["p"][1].tolist() == [0.375, 0.625]
    assert got["iterations"].tolist() == [3, 3] and got["residual"].tolist() == [0.125, 0.125]
    assert got["levels"] == [3] and got["total"] == 3 and got["active"] == [2, 2, 2] and got["reached"] == 4
    far = ppr(ap, aj, aw, [0], alpha=0.5, tol=1e-12)
    assert np.abs(far["p"][0] - [2 / 3, 1 / 3]).max() < 1e-11 and far["iterations"][0] > 30


def test_oracle_on_a_directed_path():
    """0 -> 1 -> 2: the sink is dangling and its mass returns to the seed."""
    ap, aj, aw = csr(3, [(0, 1), (1, 2)], symmetric=False)
    got = ppr(ap, aj, aw, [0, 2], alpha=0.5, tol=0, max_iterations=3, in_edges=transpose(ap, aj, aw))
    # seed 0: (1/2, 1/2, 0), (1/2, 1/4, 1/4), then D = 1/4: (1/2 + 1/8, 1/4, 1/8)
    assert got["p"][0].tolist() == [0.625, 0.25, 0.125]
    # the seed is the sink: everything it holds comes straight back
    assert got["p"][1].tolist() == [0.0, 0.0, 1.0] and got["residual"][1] == 0
    by_tol = ppr(ap, aj, aw, [0, 2], alpha=0.5, tol=2.0 ** -8, in_edges=transpose(ap, aj, aw))
    assert by_tol["iterations"][1] == 1 and by_tol["iterations"][0] > 1
    assert by_tol["levels"] == [by_tol["iterations"][0]] and by_tol["active"][:2] == [2, 1]
    assert np.allclose(by_tol["p"].sum(1), 1, atol=1e-15)


def test_transpose_of_a_symmetric_csr_is_itself():
    ap, aj, aw = csr(5, [(0, 1), (0, 2), (1, 2), (3, 4)], weights=[1, 2, 3, 4])
    tp, tj, tw = transpose(ap, aj, aw)
    a = ppr(ap, aj, aw, None, tol=0, max_iterations=9)
    b = ppr(ap, aj, aw, None, tol=0, max_iterations=9, in_edges=(tp, tj, tw))
    assert np.abs(a["p"] - b["p"]).max() < 1e-15 and a["p"].shape == (5, 5)


def test_oracle_mean_over_all_seeds_is_global_pagerank():
    ap, aj = mtx_csr(CHESAPEAKE)
    n, alpha, T = len(ap) - 1, float(np.float32(0.85)), 30
    aw = np.ones(len(aj), np.float32)
    got = ppr(ap, aj, aw, None, alpha=0.85, tol=0, max_iterations=T)
    # plain global PageRank in float64: uniform start, uniform teleport, no dangling vertex here
    degree = np.diff(ap).astype(np.float64)
    assert (degree > 0).all()
    src = np.repeat(np.arange(n), np.diff(ap))
    p = np.full(n, 1.0 / n)
    for _ in range(T):
        p = np.bincount(aj, weights=(alpha * p / degree)[src], minlength=n) + (1 - alpha) / n
    assert np.abs(got["p"].mean(0) - p).max() < 1e-12
    assert np.abs(got["p"].sum(1) - 1).max() < 1e-12 and got["levels"] == [T]


def test_oracle_matches_networkx():
    nx = pytest.importorskip("networkx")
    pytest.importorskip("scipy")
    ap, aj = mtx_csr(CHESAPEAKE)
    n = len(ap) - 1
    G = nx.DiGraph()
    G.add_nodes_from(range(n + 1))  # one isolated vertex more: dangling mass goes to the seed
    G.add_edges_from((u, int(w)) for u in range(n) for w in aj[ap[u]:ap[u + 1]])
    G.add_edge(3, n)                # ... and a sink
    edges = [(u, int(w)) for u in range(n) for w in aj[ap[u]:ap[u + 1]]] + [(3, n)]
    dp, dj, dw = csr(n + 1, edges, symmetric=False)
    seeds = [0, 3, 17, n]
    got = ppr(dp, dj, dw, seeds, alpha=0.85, tol=1e-14, in_edges=transpose(dp, dj, dw))
    for i, s in enumerate(seeds):
        want = nx.pagerank(G, alpha=float(np.float32(0.85)), personalization={s: 1}, tol=1e-15, max_iter=10000)
        assert np.abs(got["p"][i] - [want[v] for v in range(n + 1)]).max() < 1e-10


@pytest.mark.parametrize("name", sorted(exact_cases()))
def test_exact_cases_are_exact_in_float32(name):
    c = exact_cases()[name]
    kw = dict(seeds=c["seeds"], alpha=c["alpha"], tol=c["tol"], max_iterations=c["T"],
              in_edges=transpose(c["ap"], c["aj"], c["aw"]) if c["directed"] else None)
    assert exact_in_float32(c["ap"], c["aj"], c["aw"], **kw)
    got = ppr(c["ap"], c["aj"], c["aw"], **kw)
    assert (got["p"].astype(np.float32).astype(np.float64) == got["p"]).all()
    assert np.abs(got["p"].sum(1) - 1).max() == 0
    if name == "ring_isolated":
        assert got["iterations"].tolist() == [7, 1] and got["p"][1].tolist() == [0.0] * 8 + [1.0]
    if name == "star":
        assert np.diff(c["ap"]).max() == 4096


def test_exactness_check_rejects_general_floats():
    ap, aj, aw = csr(3, [(0, 1), (1, 2), (0, 2)])
    assert not exact_in_float32(ap, aj, aw, [0], alpha=0.85, tol=0, max_iterations=3)       # products of alpha / 2 need 48 bits
    ap, aj, aw = csr(4, [(0, 1), (0, 2), (0, 3)])
    assert not exact_in_float32(ap, aj, aw, [0], alpha=0.5, tol=0, max_iterations=2)        # 1 / 3


def test_rounding_bound_is_the_written_formula():
    assert rounding_bound(0, 0, 0.5) == 1.01 * 16 * 2.0 ** -24 / 0.5
    assert rounding_bound(100, 20, 0.85) == 1.01 * 136 * 2.0 ** -24 / (1 - 0.85)
