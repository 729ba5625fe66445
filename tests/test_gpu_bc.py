"""grx_bc (betweenness centrality over a list of sources) against a float64 Brandes written here:
level-synchronous over the edge arrays, np.add.at so that every parallel edge is a path of its
own, as in the reference's bc.hxx (one functor call per edge).  bc[v] = 0.5 * sum_s delta_s(v)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def brandes(ap, aj, sources):
    """(0.5 * sum over sources of delta_s, reached vertices summed over sources, last depths)."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap))
    dst = np.asarray(aj, np.int64)
    bc = np.zeros(n)
    reached = 0
    depth = None
    for s in sources:
        depth = np.full(n, -1, np.int64)
        depth[s] = 0
        sigma = np.zeros(n)
        sigma[s] = 1.0
        d = 0
        while True:
            e = depth[src] == d
            ends = dst[e]
            new = np.unique(ends[depth[ends] < 0])
            if not len(new):
                break
            depth[new] = d + 1
            e &= depth[dst] == d + 1
            np.add.at(sigma, dst[e], sigma[src[e]])
            d += 1
        delta = np.zeros(n)
        for lvl in range(d - 1, -1, -1):
            e = (depth[src] == lvl) & (depth[dst] == lvl + 1)
            u, w = src[e], dst[e]
            np.add.at(delta, u, sigma[u] / sigma[w] * (1.0 + delta[w]))
        delta[s] = 0.0
        bc += delta
        reached += int((depth >= 0).sum())
    return 0.5 * bc, reached, depth


def csr(n, edges, symmetric=True):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if symmetric:
        e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    ap = np.zeros(n + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(e[:, 0], minlength=n))
    return ap.astype(np.int32), e[:, 1].astype(np.int32)


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ap, aj):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32))


def close(got, want, rtol):
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol, atol=1e-5 * max(1.0, float(np.abs(want).max(initial=0))))


def test_chesapeake_all_sources(ea, ctx):
    mtx = os.path.join(GOLDEN_DIR, "chesapeake.mtx")
    g = ea.Graph.from_mtx(mtx)
    ap, aj, _ = g.to_host()
    want, reached, _ = brandes(ap, aj, range(g.n_rows))
    got, st = ea.bc(ctx, g)
    got = got.cpu().numpy()
    close(got, want, 1e-4)
    assert st.vertices_reached == reached
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_bc")
    if os.path.exists(exe):  # the reference harness's printed values, when it was built
        r = subprocess.run([exe, mtx], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("GPU bc values[:")][0]
        ref = np.array([float(x) for x in line.split("=")[1].split()])
        np.testing.assert_allclose(got[: len(ref)], ref, rtol=1e-3, atol=1e-3)


def _random_undirected(rng, n, m):
    return rng.integers(0, n, size=(m, 2))


SMALL = {
    "random_a": lambda rng: (40, _random_undirected(rng, 40, 80)),
    "random_b": lambda rng: (64, _random_undirected(rng, 64, 300)),
    "two_components_isolated": lambda rng: (12, [(0, 1), (1, 2), (2, 0), (2, 3), (6, 7), (7, 8), (8, 9), (7, 10)]),
    "multi_edges_self_loops": lambda rng: (7, [(0, 1), (0, 1), (1, 2), (1, 2), (1, 2), (2, 3), (3, 3), (0, 0),
                                               (3, 4), (4, 5), (1, 5), (5, 6), (6, 6), (6, 2)]),
    "path": lambda rng: (30, [(i, i + 1) for i in range(29)]),
    "star": lambda rng: (25, [(0, i) for i in range(1, 25)]),
    "single_vertex": lambda rng: (1, np.zeros((0, 2), np.int64)),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs_every_source_singly_and_as_one_list(ea, ctx, name):
    rng = np.random.default_rng(11)
    n, edges = SMALL[name](rng)
    ap, aj = csr(n, edges)
    g = graph(ea, ap, aj)
    for s in range(n):
        want, reached, _ = brandes(ap, aj, [s])
        got, st = ea.bc(ctx, g, s)
        close(got.cpu().numpy(), want, 1e-4)
        assert st.vertices_reached == reached
    want, _, _ = brandes(ap, aj, range(n))
    close(ea.bc(ctx, g)[0].cpu().numpy(), want, 1e-4)
    close(ea.bc(ctx, g, np.arange(n))[0].cpu().numpy(), want, 1e-4)
    if n >= 2:  # the same on a hot-first renumbered copy
        g.hot_first(ctx, True)
        close(ea.bc(ctx, g)[0].cpu().numpy(), want, 1e-4)


def test_duplicate_sources_count_twice(ea, ctx):
    ap, aj = csr(30, [(i, i + 1) for i in range(29)])
    g = graph(ea, ap, aj)
    want, _, _ = brandes(ap, aj, [5, 5, 17])
    close(ea.bc(ctx, g, [5, 5, 17])[0].cpu().numpy(), want, 1e-4)


def test_directed_graph_needs_in_edges(ea, ctx):
    rng = np.random.default_rng(5)
    n = 50
    edges = rng.integers(0, n, size=(200, 2))
    ap, aj = csr(n, edges, symmetric=False)
    g = graph(ea, ap, aj)
    with pytest.raises(ea.EngineError) as e:
        ea.bc(ctx, g, 0)
    assert e.value.code == -3
    g.build_in_edges(ctx)
    for s in range(n):
        want, reached, _ = brandes(ap, aj, [s])
        got, st = ea.bc(ctx, g, s)
        close(got.cpu().numpy(), want, 1e-4)
        assert st.vertices_reached == reached
    want, _, _ = brandes(ap, aj, range(n))
    close(ea.bc(ctx, g)[0].cpu().numpy(), want, 1e-4)


def test_argument_errors_and_empty_list(ea, ctx):
    ap, aj = csr(10, [(i, i + 1) for i in range(9)])
    g = graph(ea, ap, aj)
    for bad in ([10], [-1], [3, 11]):
        with pytest.raises(ea.EngineError) as e:
            ea.bc(ctx, g, bad)
        assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.bc(ctx, g, 0, options=ea.Options(max_iterations=2))
    assert e.value.code == -1
    import torch
    out = torch.full((10,), 7.0, dtype=torch.float32, device="cuda")
    got, st = ea.bc(ctx, g, np.zeros(0, np.int32), bc_values=out)
    assert (got.cpu().numpy() == 0).all() and st.vertices_reached == 0


def test_deterministic_on_rmat16(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    deg = np.diff(g.offsets_to_host())
    sources = np.random.default_rng(3).choice(np.flatnonzero(deg > 0), 8)
    a, _ = ea.bc(ctx, g, sources)
    a = a.clone()
    b, _ = ea.bc(ctx, g, sources)
    assert torch.equal(a, b)
    g.hot_first(ctx, False)  # the caller's numbering: another summation order
    c, _ = ea.bc(ctx, g, sources)
    close(c.cpu().numpy(), a.cpu().numpy().astype(np.float64), 1e-4)


def test_rmat18_sampled_sources(ea, ctx):
    g = ea.Graph.rmat(ctx, 18, 16, 1, 7)
    ap, aj, _ = g.to_host()
    deg = np.diff(ap)
    sources = [int(x) for x in np.random.default_rng(7).choice(np.flatnonzero(deg > 0), 4)]
    want, reached, _ = brandes(ap, aj, sources)
    got, st = ea.bc(ctx, g, sources)
    close(got.cpu().numpy(), want, 1e-3)
    assert st.vertices_reached == reached


def test_rmat22_two_sources_invariants(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
    deg = np.diff(g.offsets_to_host())
    sources = [0, int(np.random.default_rng(100).choice(np.flatnonzero(deg > 0)))]
    got, st = ea.bc(ctx, g, sources)
    got = got.cpu().numpy()
    want_sum, reached_any = 0.0, np.zeros(g.n_rows, bool)
    d = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
    for s in sources:
        depth = ea.bfs(ctx, g, s, d)[0].cpu().numpy().astype(np.int64)
        r = depth != ea.INT_UNREACHED
        r[s] = False
        want_sum += float((depth[r] - 1).sum())
        reached_any |= depth != ea.INT_UNREACHED
    assert np.isclose(got.astype(np.float64).sum(), 0.5 * want_sum, rtol=1e-3)
    assert (got[deg <= 1] == 0).all()
    assert (got[~reached_any] == 0).all()
    assert (got >= 0).all()
