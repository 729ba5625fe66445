"""grx_hits (two pull products per iteration, normalised by the largest magnitude) against the float64
oracle of tests/hits_oracle.py: bit for bit where float32 is exact, within the derived rounding bound
elsewhere.  Every call is made twice and must repeat itself.  Each case is named for what can go wrong
at its shape."""
import ctypes as C
import os

import numpy as np
import pytest

from hits_oracle import case_in_edges, csr, exact_cases, hits, rounding_bound, transpose

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
CASES = exact_cases()


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ctx, ap, aj, aw, directed=False, n_cols=None):
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols)
    return g.build_in_edges(ctx) if directed else g


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def twice(ea, ctx, g, tol, T=0):
    """Two calls of ea.hits into tensors filled with something else: the second repeats the first bit
    for bit.  -> (h, a as numpy arrays, info, Stats) of the first."""
    import torch
    first = None
    for fill in (-7.0, float("nan")):
        mine = torch.full((2, g.n_rows), fill, dtype=torch.float32, device="cuda")
        h, a, info, st = ea.hits(ctx, g, tol=tol, hubs=mine[0], authorities=mine[1],
                                 options=ea.Options(max_iterations=T))
        assert h.data_ptr() == mine[0].data_ptr() and a.data_ptr() == mine[1].data_ptr()
        assert st.iterations == info["iterations"]
        assert st.edges_traversed == st.edges_expanded == 2 * g.nnz * info["iterations"]
        assert st.vertices_reached == int(((h > 0) | (a > 0)).sum())
        assert st.elapsed_ms > 0 and st.advance_kernel_ms == 0
        got = (h.cpu().numpy(), a.cpu().numpy(), info, st)
        if first is None:
            first = got
        else:
            assert (bits(got[0]) == bits(first[0])).all() and (bits(got[1]) == bits(first[1])).all()
            assert info["iterations"] == first[2]["iterations"]
            assert bits(info["residual"]) == bits(first[2]["residual"])
            assert st.advance_launches == first[3].advance_launches
    return first


# ---- where float32 is exact: the oracle bit for bit ------------------------------------------------

def check_exact(ea, ctx, name):
    c = CASES[name]
    want = hits(c["ap"], c["aj"], c["aw"], c["tol"], c["T"], in_edges=case_in_edges(c))
    g = graph(ea, ctx, c["ap"], c["aj"], c["aw"], c["directed"])
    h, a, info, st = twice(ea, ctx, g, c["tol"], c["T"])
    assert (bits(h) == bits(want["h"])).all(), np.abs(h - want["h"]).max()
    assert (bits(a) == bits(want["a"])).all(), np.abs(a - want["a"]).max()
    assert info["iterations"] == want["iterations"]
    assert bits(info["residual"]) == bits(want["residual"])
    assert st.vertices_reached == want["reached"] and st.edges_traversed == want["edges"]
    return h, a, info


@pytest.mark.parametrize("name", ["ring", "two_edges", "k24_plus_edge", "path_w"])
def test_exact_on_small_graphs(ea, ctx, name):
    h, a, info = check_exact(ea, ctx, name)
    if name == "two_edges":
        assert h.tolist() == [1.0, 0.0, 2.0 ** -10, 0.0] and a.tolist() == [0.0, 1.0, 0.0, 2.0 ** -9]
        assert info == {"iterations": 5, "residual": 3 / 1024}
    if name == "path_w":
        assert h.tolist() == [1.0, 2.0 ** -12, 2.0 ** -24, 0.0] and info["iterations"] == 6


@pytest.mark.parametrize("segment", [None, "64"])
@pytest.mark.parametrize("name", ["out_star", "in_star"])
def test_exact_on_a_star_whose_hub_row_is_cut(ea, ctx, monkeypatch, name, segment):
    """A row (out_star) or an in-row (in_star) of 4096 entries: 8 partial sums by default, 64 with the
    hook at its minimum, added in segment order; V = 4097 is no multiple of a workgroup's 16 rows."""
    if segment:
        monkeypatch.setenv("GRX_SPMV_SEGMENT", segment)
    h, a, info = check_exact(ea, ctx, name)
    assert info == {"iterations": 2, "residual": 0.0}
    centre, leaves = (h, a) if name == "out_star" else (a, h)
    assert centre.tolist() == [1.0] + [0.0] * 4096 and leaves.tolist() == [0.0] + [1.0] * 4096


# ---- general floats: within the derived bound ----------------------------------------------------------

def check_bound(ea, ctx, g, ap, aj, aw, in_edges, T):
    want = hits(ap, aj, aw, 0.0, T, in_edges=in_edges)
    D = int(max(np.diff(ap).max(), np.diff(ap if in_edges is None else in_edges[0]).max()))
    bound = rounding_bound(T, D)
    h, a, info, _ = twice(ea, ctx, g, 0.0, T)
    eh, ea_ = np.abs(h.astype(np.float64) - want["h"]).max(), np.abs(a.astype(np.float64) - want["a"]).max()
    er = abs(float(info["residual"]) - want["residual"])
    print(f"T {T}, D {D}: hub error {eh:.3e}, authority error {ea_:.3e}, residual error {er:.3e}, bound {bound:.3e}")
    assert info["iterations"] == T == want["iterations"]
    assert eh <= bound and ea_ <= bound and er <= 2 * bound
    assert 1 - bound <= h.max() <= 1 and 1 - bound <= a.max() <= 1
    return h, a, info


@pytest.fixture(scope="module")
def chesapeake(ea):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, aw = g.to_host()
    assert g.n_rows == 39 and np.diff(ap).max() == 33
    return g, ap, aj, aw


@pytest.mark.parametrize("T", [1, 4, 16])
def test_chesapeake_within_the_bound(ea, ctx, chesapeake, T):
    """Symmetric, no in-edges: the rows serve both products."""
    g, ap, aj, aw = chesapeake
    check_bound(ea, ctx, g, ap, aj, aw, None, T)


@pytest.mark.parametrize("T", [1, 4, 16])
def test_a_weighted_random_digraph_within_the_bound(ea, ctx, T):
    rng = np.random.default_rng(200)
    pairs = sorted({(int(u), int(v)) for u, v in rng.integers(0, 200, (1200, 2)) if u != v})
    ap, aj, aw = csr(200, pairs, rng.integers(1, 65, len(pairs)), symmetric=False)
    g = graph(ea, ctx, ap, aj, aw, directed=True)
    check_bound(ea, ctx, g, ap, aj, aw, transpose(ap, aj, aw), T)


def test_a_directed_rmat_within_the_bound(ea, ctx):
    """A multigraph with loops as generated, hub rows and hub in-rows beyond one segment, empty rows."""
    g = ea.Graph.rmat(ctx, 10, 8, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    check_bound(ea, ctx, g, ap, aj, aw, transpose(ap, aj, aw), 8)


# ---- stopping by tol -----------------------------------------------------------------------------------

def test_stops_at_the_first_residual_below_tol(ea, ctx, chesapeake):
    g, ap, aj, aw = chesapeake
    tol = 1e-4
    h, a, info, st = twice(ea, ctx, g, tol)
    t = info["iterations"]
    assert t > 2 and info["residual"] < tol
    _, _, before, _ = twice(ea, ctx, g, 0.0, t - 1)
    assert before["iterations"] == t - 1 and before["residual"] >= tol
    want = hits(ap, aj, aw, 0.0, t)
    bound = rounding_bound(t, 33)
    print(f"stopped at {t}: residual {info['residual']:.3e}, the oracle's {want['residual']:.3e}, bound {bound:.3e}")
    assert abs(float(info["residual"]) - want["residual"]) <= 2 * bound
    # ... and the cap does not change what an iteration computes
    same, _, capped, _ = twice(ea, ctx, g, 0.0, t)
    assert (bits(same) == bits(h)).all() and bits(capped["residual"]) == bits(info["residual"])
    normalized = ea.hits(ctx, g, tol=tol, normalized=True)
    assert abs(float(normalized[0].double().sum()) - 1) < 1e-6 and abs(float(normalized[1].double().sum()) - 1) < 1e-6
    assert np.allclose(normalized[0].cpu().numpy(), h / h.astype(np.float64).sum(), rtol=1e-6, atol=0)


# ---- edge cases ------------------------------------------------------------------------------------------

def test_one_output_at_a_time(ea, ctx, chesapeake):
    import torch
    from essentials_amd.api import load_library, _Options
    lib = load_library()
    g, ap, aj, aw = chesapeake
    h, a, info, _ = twice(ea, ctx, g, 0.0, 7)
    o = ea.Options(max_iterations=7)._c()
    out = torch.full((39,), -7.0, dtype=torch.float32, device="cuda")
    t, r = C.c_int32(), C.c_float()
    assert lib.grx_hits(ctx._h, g._h, 0.0, out.data_ptr(), None, C.byref(t), C.byref(r), C.byref(o), None) == 0
    assert (bits(out.cpu().numpy()) == bits(h)).all() and t.value == 7 and bits(r.value) == bits(info["residual"])
    assert lib.grx_hits(ctx._h, g._h, 0.0, None, out.data_ptr(), None, None, C.byref(o), None) == 0
    assert (bits(out.cpu().numpy()) == bits(a)).all()
    assert isinstance(o, _Options)


def test_no_entries_follows_the_definition(ea, ctx):
    ap, aj, aw = csr(5, [])
    h, a, info, st = twice(ea, ctx, graph(ea, ctx, ap, aj, aw), 2.0 ** -8)
    assert h.tolist() == [0.0] * 5 and a.tolist() == [0.0] * 5
    assert info == {"iterations": 2, "residual": 0.0} and st.vertices_reached == 0 and st.edges_traversed == 0


def test_no_vertices(ea, ctx):
    g = ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])
    h, a, info, st = ea.hits(ctx, g)
    assert h.numel() == 0 and a.numel() == 0 and info == {"iterations": 0, "residual": 0.0}
    assert st.iterations == 0 and st.advance_launches == 0 and st.elapsed_ms == 0


def test_the_clocks(ea, ctx, chesapeake):
    g = chesapeake[0]
    for tol, T in ((0.0, 5), (1e-4, 0)):
        _, _, info, st = ea.hits(ctx, g, tol=tol, options=ea.Options(collect_kernel_time=True, max_iterations=T))
        assert 0 < st.advance_kernel_ms <= st.elapsed_ms
        assert st.advance_launches >= 2 * info["iterations"] + 2


# ---- errors ----------------------------------------------------------------------------------------------

def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    v = np.arange(9)
    ap, aj, aw = csr(10, np.concatenate([np.stack([v, v + 1], 1), [[9, 0], [5, 2]]]), symmetric=False)
    g = graph(ea, ctx, ap, aj, aw, directed=True)

    def refused(code, **kw):
        with pytest.raises(ea.EngineError) as e:
            ea.hits(ctx, kw.pop("on", g), **kw)
        assert e.value.code == code and b"grx_hits" in lib.grx_last_error()

    refused(-1, on=graph(ea, ctx, ap, aj, aw, n_cols=11))
    refused(-1, tol=float("nan"))
    refused(-1, tol=0.0)
    refused(-1, tol=-1.0)
    refused(-1, options=ea.Options(max_iterations=-1))
    out = torch.full((10,), -7.0, dtype=torch.float32, device="cuda")
    assert lib.grx_hits(ctx._h, g._h, 1e-6, None, None, None, None, None, None) == -1
    assert b"both NULL" in lib.grx_last_error()
    assert lib.grx_hits(None, g._h, 1e-6, out.data_ptr(), None, None, None, None, None) == -1
    assert lib.grx_hits(ctx._h, None, 1e-6, out.data_ptr(), None, None, None, None, None) == -1
    ctx.synchronize()
    assert (out == -7).all()
    # ... and the same arguments put right
    assert lib.grx_hits(ctx._h, g._h, 1e-6, out.data_ptr(), None, None, None, None, None) == 0
    assert 0.999 < float(out.max()) <= 1 and float(out.min()) >= 0
    with pytest.raises(TypeError):
        ea.hits(ctx, g, hubs=out.double())
    with pytest.raises(ValueError):
        ea.hits(ctx, g, authorities=out[:-1])


def test_an_asymmetric_csr_needs_in_edges(ea, ctx):
    from essentials_amd.api import load_library
    lib = load_library()
    c = CASES["path_w"]
    g = graph(ea, ctx, c["ap"], c["aj"], c["aw"])
    with pytest.raises(ea.EngineError) as e:
        ea.hits(ctx, g, tol=0.0, options=ea.Options(max_iterations=6))
    message = lib.grx_last_error()
    assert e.value.code == -3 and b"grx_hits" in message and b"grx_graph_build_in_edges" in message
    g.build_in_edges(ctx)
    h, _, info, _ = ea.hits(ctx, g, tol=0.0, options=ea.Options(max_iterations=6))
    assert h.tolist() == [1.0, 2.0 ** -12, 2.0 ** -24, 0.0] and info["iterations"] == 6
