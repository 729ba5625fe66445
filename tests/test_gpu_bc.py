"""grx_bc (betweenness centrality over a list of sources) against tests/bc_oracle.py: a float64
Brandes, level-synchronous over the edge arrays, np.add.at so that every parallel edge is a path of
its own, as in the reference's bc.hxx (one functor call per edge).  bc[v] = 0.5 * sum_s delta_s(v).

Two comparisons per vertex, neither with an absolute tolerance: bit for bit against
bc_oracle.bc_order_free on graphs where no order of the additions can change a bit (rows at the
kernels' own thresholds: BC_HUB = 256, BC_CHUNK = 2048, the grids of the two sweeps), and
|got - want| <= gamma(K[v]) want[v] with brandes64's rounding count K elsewhere.
tests/test_bc_oracle.py checks both references on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import bc_oracle as bo
from bc_oracle import csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


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


class Worst:
    """Every vertex within gamma(K[v]) want[v] of the float64 value (+0 where that is 0); the largest
    error / bound of a test is printed when it ends."""

    def __init__(self, what):
        self.what, self.top = what, 0.0

    def __call__(self, got, want, K, where=""):
        r = bo.within_bound(got, want, K)
        self.top = max(self.top, r)
        assert r <= 1.0, (self.what, where, r)

    def report(self):
        print(f"{self.what}: largest error / bound {self.top:.3f}")


def test_chesapeake_all_sources(ea, ctx):
    mtx = os.path.join(GOLDEN_DIR, "chesapeake.mtx")
    g = ea.Graph.from_mtx(mtx)
    ap, aj, _ = g.to_host()
    want, reached, _, _, K = bo.brandes64(ap, aj, range(g.n_rows))
    got, st = ea.bc(ctx, g)
    got = got.cpu().numpy()
    close(got, want, 1e-4)
    bound = Worst("chesapeake, every source")
    bound(got, want, K)
    bound.report()
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
    bound = Worst(name)
    for s in range(n):
        want, reached, _, _, K = bo.brandes64(ap, aj, [s])
        got, st = ea.bc(ctx, g, s)
        close(got.cpu().numpy(), want, 1e-4)
        bound(got.cpu().numpy(), want, K, s)
        assert st.vertices_reached == reached
    want, _, _, _, K = bo.brandes64(ap, aj, range(n))
    for sources in (None, np.arange(n)):
        got = ea.bc(ctx, g, sources)[0].cpu().numpy()
        close(got, want, 1e-4)
        bound(got, want, K, "every source")
    if n >= 2:  # the same on a hot-first renumbered copy
        g.hot_first(ctx, True)
        got = ea.bc(ctx, g)[0].cpu().numpy()
        close(got, want, 1e-4)
        bound(got, want, K, "hot first")
    bound.report()


def test_duplicate_sources_count_twice(ea, ctx):
    ap, aj = csr(30, [(i, i + 1) for i in range(29)])
    g = graph(ea, ap, aj)
    want, _, _, _, K = bo.brandes64(ap, aj, [5, 5, 17])
    got = ea.bc(ctx, g, [5, 5, 17])[0].cpu().numpy()
    close(got, want, 1e-4)
    bound = Worst("duplicate sources")
    bound(got, want, K)
    bound.report()


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
    bound = Worst("directed, 50 vertices")
    for s in range(n):
        want, reached, _, _, K = bo.brandes64(ap, aj, [s])
        got, st = ea.bc(ctx, g, s)
        close(got.cpu().numpy(), want, 1e-4)
        bound(got.cpu().numpy(), want, K, s)
        assert st.vertices_reached == reached
    want, _, _, _, K = bo.brandes64(ap, aj, range(n))
    got = ea.bc(ctx, g)[0].cpu().numpy()
    close(got, want, 1e-4)
    bound(got, want, K, "every source")
    bound.report()


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
    want, reached, _, _, K = bo.brandes64(ap, aj, sources)
    got, st = ea.bc(ctx, g, sources)
    close(got.cpu().numpy(), want, 1e-3)
    bound = Worst("rmat18, 4 sources")
    bound(got.cpu().numpy(), want, K)
    bound.report()
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


# ---------------------------------------------------------------------------
# per vertex: hub rows, chunk boundaries, launch shapes, path counts far from 1
# ---------------------------------------------------------------------------
BIT = bo.bit_cases()


def run_twice(ea, ctx, g, sources, stats, options=None):
    """grx_bc into outputs prefilled with -7 and then NaN (d_bc is overwritten, not added to): the
    two results agree bit for bit, and the stats are the oracle's sums over sources."""
    import torch
    got = []
    for fill in (-7.0, float("nan")):
        out = torch.full((g.n_rows,), fill, dtype=torch.float32, device="cuda")
        res, st = ea.bc(ctx, g, sources, bc_values=out, options=options)
        assert res is out
        assert (st.vertices_reached, st.edges_traversed, st.iterations) == stats, (fill, options)
        got.append(out.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes()
    return got[0]


def numberings(ea, ctx, ap, aj, symmetric):
    """The graph on the caller's numbering and, when it is symmetric, renumbered hot first (a
    directed graph with attached in-edges keeps the caller's numbering)."""
    g = graph(ea, ap, aj)
    if not symmetric:
        g.build_in_edges(ctx)
        yield "caller's numbering", g
    else:
        g.hot_first(ctx, False)
        yield "caller's numbering", g
        g.hot_first(ctx, True)
        yield "hot first", g


def same_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), (what, len(bad), bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


def check_bit_for_bit(ea, ctx, name, ap, aj, sources, symmetric):
    want, free = bo.bc_order_free(ap, aj, sources)
    assert free, name
    _, reached, edges, levels, _ = bo.brandes64(ap, aj, sources)
    for where, g in numberings(ea, ctx, ap, aj, symmetric):
        same_bits(run_twice(ea, ctx, g, sources, (reached, edges, levels)), want, (name, where))


@pytest.mark.parametrize("name", list(BIT))
def test_hub_and_chunk_boundaries_bit_for_bit(ea, ctx, name):
    """Rows of 255 .. 4097 edges in either sweep, slots sized by the longer direction of a directed
    hub, parallel edges into hub rows, sigma = 2^100: no order of the additions changes a bit of
    these (tests/test_bc_oracle.py), so every vertex must match bc_order_free exactly."""
    check_bit_for_bit(ea, ctx, name, *BIT[name]())


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_level_wider_than_one_trip_of_the_level_kernel(ea, ctx):
    """More rows on one level than bc_level_kernel's grid (8 workgroups per CU) has lane groups: a
    second trip, whose last lane groups lie past the level's end."""
    ap, aj, sources, rows, groups = bo.wide_level_case(compute_units())
    print(f"{compute_units()} CUs: {rows} rows on one level, {groups} lane groups per trip")
    assert groups < rows < 2 * groups and rows % groups
    check_bit_for_bit(ea, ctx, f"out_fan{rows}", ap, aj, sources, True)


@pytest.mark.parametrize("directed", [False, True])
def test_more_chunk_slots_than_workgroups_of_the_chunk_kernel(ea, ctx, directed):
    """More hub rows of in-degree 256 on one level than bc_hub_chunk_kernel's grid has workgroups:
    a workgroup loops over several slots."""
    ap, aj, sources, slots, grid = bo.many_slots_case(compute_units(), directed)
    print(f"{compute_units()} CUs: {slots} chunk slots on one level, {grid} workgroups, {len(aj)} edges")
    assert slots > grid
    check_bit_for_bit(ea, ctx, f"bipartite_layer256_{slots}", ap, aj, sources, not directed)


FUNNELS = [(255, 257), (300, 10), (2049, 255)]


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("m1,m2", FUNNELS)
def test_funnels_per_vertex_bound(ea, ctx, m1, m2, directed):
    """Hub rows whose sums do round: every vertex within gamma(K[v]) of the float64 value."""
    ap, aj, ids = bo.funnel(m1, m2, directed=directed)
    sources = [ids["s"]] if directed else [ids["s"], int(ids["A"][0]), ids["h"], int(ids["B"][-1]), ids["t"]]
    want, reached, edges, levels, K = bo.brandes64(ap, aj, sources)
    bound = Worst(f"funnel({m1}, {m2}) directed={directed}")
    for where, g in numberings(ea, ctx, ap, aj, not directed):
        bound(run_twice(ea, ctx, g, sources, (reached, edges, levels)), want, K, where)
    bound.report()


@pytest.mark.parametrize("symmetric", [True, False])
def test_rmat10_per_vertex_bound_under_every_option(ea, ctx, oracle, symmetric):
    """A power-law graph with hub rows, 72 sources: the per-vertex bound (no atol: a quarter of the
    vertices lie below the 1e-5 max|bc| that close() forgives), and the options of the depth search
    change no bit of the result."""
    n, ap, aj, _ = oracle.rmat_csr(10, 16, 1, 7, symmetric)
    aj = np.ascontiguousarray(aj)
    out, into = np.diff(ap), np.bincount(aj, minlength=n)
    assert max(out.max(), into.max()) >= bo.BC_HUB
    busy = np.flatnonzero((out > 0) | (into > 0))
    sources = np.concatenate([np.random.default_rng(21).choice(busy, 64, replace=False),
                              np.argsort(-np.maximum(out, into), kind="stable")[:8]])
    want, reached, edges, levels, K = bo.brandes64(ap, aj, sources)
    small = (want > 0) & (want < 1e-5 * want.max())
    print(f"rmat10 symmetric={symmetric}: {small.mean():.0%} of the vertices have 0 < bc < 1e-5 max|bc|, "
          f"largest gamma(K) {bo.gamma(K.max()):.2e}")
    bound = Worst(f"rmat10 symmetric={symmetric}, 72 sources")
    stats = (reached, edges, levels)
    first = None
    for where, g in numberings(ea, ctx, ap, aj, symmetric):
        got = run_twice(ea, ctx, g, sources, stats)
        bound(got, want, K, where)
        close(got, want, 1e-4)
        if first is None:
            first = got
            options = [ea.Options(load_balance=lb) for lb in ea.LoadBalance] + [ea.Options(call_every_edge=True)]
            for o in options:
                same_bits(run_twice(ea, ctx, g, sources, stats, o), first, (where, o))
    bound.report()
