"""CPU checks of HITS' and SpMV's place in the product boundary (the header declares grx_hits and
grx_spmv, the library exports them, the Python layer offers essentials_amd.hits and .spmv) and of the
oracle the GPU tests compare against (tests/hits_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hits_oracle import case_in_edges, csr, exact_cases, exact_in_float32, hits, rounding_bound, spmv, transpose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CASES = exact_cases()


def run(name):
    c = CASES[name]
    return hits(c["ap"], c["aj"], c["aw"], c["tol"], c["T"], in_edges=case_in_edges(c))


def test_header_declares_both_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_spmv\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*int32_t\s+transpose,"
                     r"\s*const\s+float\s*\*\s*d_x,\s*float\s*\*\s*d_y,\s*const\s+grx_options\s*\*\s*opt,"
                     r"\s*grx_stats\s*\*\s*stats\s*\)", text)
    assert re.search(r"\bint\s+grx_hits\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*float\s+tol,"
                     r"\s*float\s*\*\s*d_hub,\s*float\s*\*\s*d_authority,\s*int32_t\s*\*\s*h_iterations,"
                     r"\s*float\s*\*\s*h_residual,\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)",
                     text)
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", text)


def test_library_exports_both_calls():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_hits") and hasattr(lib, "grx_spmv")


def test_python_layer_offers_hits_and_spmv():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.hits) and callable(ea.spmv)
    assert "hits" in ea.__all__ and "spmv" in ea.__all__
    assert "grx_hits" in _SIGNATURES and "grx_spmv" in _SIGNATURES


# ---- the oracle gives the hand values ------------------------------------------------------------------

def test_ring_stops_at_once():
    got = run("ring")
    assert got["iterations"] == 1 and got["residuals"] == [0.0]
    assert got["h"].tolist() == [1.0] * 8 and got["a"].tolist() == [1.0] * 8
    assert got["edges"] == 2 * 16 and got["reached"] == 8


def test_two_edges():
    got = run("two_edges")
    assert got["iterations"] == 5
    assert got["h"].tolist() == [1.0, 0.0, 2.0 ** -10, 0.0] and got["a"].tolist() == [0.0, 1.0, 0.0, 2.0 ** -9]
    assert got["residuals"] == [1.0, 3 / 16, 3 / 64, 3 / 256, 3 / 1024] and got["residual"] == 3 / 1024
    assert got["reached"] == 4 and got["edges"] == 2 * 2 * 5


def test_k24_plus_edge():
    got = run("k24_plus_edge")
    assert got["iterations"] == 5 and got["residual"] == 7 * 2.0 ** -15
    assert got["h"][:2].tolist() == [1.0, 1.0] and got["a"][2:6].tolist() == [1.0] * 4
    assert 0 < got["h"][6] < 2.0 ** -10 and got["h"][7] == 0 and got["a"][6] == 0


def test_stars():
    out, into = run("out_star"), run("in_star")
    assert out["iterations"] == 2 and out["residuals"] == [1.0, 0.0]
    assert out["h"].tolist() == [1.0] + [0.0] * 4096 and out["a"].tolist() == [0.0] + [1.0] * 4096
    assert np.diff(CASES["out_star"]["ap"]).max() == 4096
    # the mirror image: hubs and authorities change places
    assert into["iterations"] == 2 and into["residuals"] == [1.0, 0.0]
    assert into["a"].tolist() == out["h"].tolist() and into["h"].tolist() == out["a"].tolist()
    assert np.diff(case_in_edges(CASES["in_star"])[0]).max() == 4096


def test_weighted_path():
    got = run("path_w")
    assert got["iterations"] == 6
    assert got["a"].tolist() == [0.0, 1.0, 2.0 ** -11, 2.0 ** -22]
    assert got["h"].tolist() == [1.0, 2.0 ** -12, 2.0 ** -24, 0.0]


def test_no_entries_follows_the_definition():
    ap, aj, aw = csr(5, [])
    got = hits(ap, aj, aw, 2.0 ** -8)
    assert got["iterations"] == 2 and got["residuals"] == [1.0, 0.0]
    assert not got["a"].any() and not got["h"].any() and got["reached"] == 0 and got["edges"] == 0
    assert hits(ap[:1], aj, aw, 2.0 ** -8)["iterations"] == 0   # V == 0


def test_a_symmetric_csr_is_its_own_in_edges():
    ap, aj, aw = csr(5, [(0, 1), (0, 2), (1, 2), (3, 4)], weights=[1, 2, 3, 4])
    a = hits(ap, aj, aw, 0, 9)
    b = hits(ap, aj, aw, 0, 9, in_edges=transpose(ap, aj, aw))
    assert np.abs(a["a"] - b["a"]).max() < 1e-15 and np.abs(a["h"] - b["h"]).max() < 1e-15


# ---- exactness -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_cases_are_exact_in_float32(name):
    c = CASES[name]
    assert exact_in_float32(c["ap"], c["aj"], c["aw"], c["tol"], c["T"], in_edges=case_in_edges(c))
    got = run(name)
    for v in (got["a"], got["h"], np.array(got["residuals"])):
        assert (v.astype(np.float32).astype(np.float64) == v).all()
    assert max(got["a"].max(), got["h"].max()) == 1


def test_exactness_check_rejects_a_third():
    ap, aj, aw = csr(4, [(0, 1), (0, 2), (0, 3), (1, 2)])
    # vertex 0 sums to 3 where 1 and 2 sum to 2: the scaled vector holds 2 / 3 and 1 / 3
    assert not exact_in_float32(ap, aj, aw, 0, 2)
    ap, aj, aw = csr(3, [(0, 1), (0, 2)], weights=[1 / 3, 1.0], symmetric=False)
    assert not exact_in_float32(ap, aj, aw, 0, 2, in_edges=transpose(ap, aj, aw))  # a weight of 1 / 3 beside 1


def test_rounding_bound_is_the_written_formula():
    assert rounding_bound(1, 0) == 1.01 * 13 * 2.0 ** -24
    assert rounding_bound(16, 33) == 1.01 * (4 * 16 * 36 + 1) * 2.0 ** -24


# ---- the oracle's products and another implementation ----------------------------------------------------

def test_oracle_spmv():
    ap, aj, aw = csr(3, [(0, 1), (0, 3), (2, 0)], weights=[2, 3, 5], symmetric=False)  # 3 x 4
    x = np.array([1.0, 10.0, 100.0, 1000.0])
    assert spmv(ap, aj, aw, x).tolist() == [3020.0, 0.0, 5.0]
    assert spmv(ap, aj, aw, x[:3], n_cols=4, transpose=True).tolist() == [500.0, 2.0, 0.0, 3.0]


def test_oracle_matches_networkx():
    nx = pytest.importorskip("networkx")
    pytest.importorskip("scipy")
    rng = np.random.default_rng(5)
    n = 60
    pairs = sorted({(int(u), int(v)) for u, v in rng.integers(0, n, (400, 2)) if u != v})
    weights = rng.integers(1, 65, len(pairs)).astype(np.float64)
    ap, aj, aw = csr(n, pairs, weights, symmetric=False)
    got = hits(ap, aj, aw, 1e-15, 5000, in_edges=transpose(ap, aj, aw))
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from((u, v, w) for (u, v), w in zip(pairs, weights))
    hubs, authorities = nx.hits(G, max_iter=10000, tol=1e-15)
    for mine, theirs in ((got["h"], hubs), (got["a"], authorities)):
        error = np.abs(mine / mine.sum() - [theirs[v] for v in range(n)]).max()
        print(f"largest difference from networkx.hits: {error:.1e}")
        assert error < 1e-12
