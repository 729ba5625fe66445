"""grx_scc (strongly connected components) against the Tarjan oracle of tests/scc_oracle.py,
exactly: known answers, chesapeake, directed R-MAT in several layouts, shapes that stress the
schedule (thousands of narrow trim generations and reach levels, many rounds, rows above the big-row
threshold) in three numberings, the test hooks, the stats, argument errors and invariants on
RMAT-18.  The label of a vertex is the smallest vertex id of its component."""
import ctypes as C
import os

import numpy as np
import pytest

from scc_oracle import KNOWN, csr, known_csr, strong_components

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, want, count, directed=True, options=None):
    """ea.scc(g) gives `want` exactly; the stats are the answer's.  directed: the call walks both
    arrays itself (in-edges attached) rather than handing the graph to grx_cc."""
    labels, got, st = ea.scc(ctx, g, options=options)
    assert str(labels.dtype) == "torch.int32" and labels.numel() == g.n_rows
    host = labels.cpu().numpy()
    print(f"V {g.n_rows} nnz {g.nnz} components {got} iterations {st.iterations} edges_expanded {st.edges_expanded} "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
    assert (host == want).all()
    assert got == count == int((host == np.arange(g.n_rows)).sum())
    assert st.vertices_reached == g.n_rows - count
    assert st.edges_expanded == st.edges_traversed
    if directed:
        # a recount of at most both rows of every vertex per round and the first one, at most both
        # rows of every vertex per round of reach, every vertex trimmed once
        assert 0 <= st.edges_expanded <= 2 * g.nnz * (2 * st.iterations + 2)
        if g.n_rows:
            assert st.advance_launches > 0
    return labels, st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, want = known_csr(name)
    oracle = strong_components(ap, aj)
    assert oracle[0].tolist() == want.tolist()
    labels, _ = check(ea, ctx, graph(ea, ap, aj).build_in_edges(ctx), *oracle)
    assert labels.cpu().numpy().tolist() == want.tolist()
    if KNOWN[name][2]:  # symmetric: every edge runs both ways, no in-edges needed
        labels, _ = check(ea, ctx, graph(ea, ap, aj), *oracle, directed=False)
        assert labels.cpu().numpy().tolist() == want.tolist()


def test_chesapeake(ea, ctx):
    import torch
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    weak, _, _ = ea.cc(ctx, g)
    weak = weak.clone()
    labels, _ = check(ea, ctx, g, *strong_components(ap, aj), directed=False)
    assert g.n_rows == 39 and torch.equal(labels, weak)
    g.build_in_edges(ctx)
    again, st = check(ea, ctx, g, *strong_components(ap, aj))
    assert torch.equal(again, weak) and st.iterations >= 1
    # its strictly upper-triangular entries: a DAG, which trimming alone finishes
    src = np.repeat(np.arange(39, dtype=np.int64), np.diff(ap))
    upper = src < aj
    dag = graph(ea, *csr(39, np.stack([src[upper], aj[upper].astype(np.int64)], 1), symmetric=False)).build_in_edges(ctx)
    _, st = check(ea, ctx, dag, np.arange(39, dtype=np.int32), 39)
    assert st.iterations == 0


@pytest.mark.parametrize("scale", [10, 14, 16])
def test_directed_rmat_in_every_layout(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=False)
    ap, aj, _ = g.to_host()
    want, count = strong_components(ap, aj)
    assert 1 < count < g.n_rows
    labels, _ = check(ea, ctx, g.build_in_edges(ctx), want, count)
    labels = labels.clone()
    for other in (g.sorted_rows(ctx), g.simple(ctx)):
        check(ea, ctx, other.build_in_edges(ctx), want, count)
    again, count2, _ = ea.scc(ctx, g)
    assert torch.equal(again, labels) and count2 == count
    # a hot-first copy on the handle (built before the in-edges: they fix the numbering) is not used
    hot = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=False).hot_first(ctx, True).build_in_edges(ctx)
    again, count3, _ = ea.scc(ctx, hot)
    assert torch.equal(again, labels) and count3 == count


def _ring(n=5000):
    v = np.arange(n, dtype=np.int64)
    return n, np.stack([v, (v + 1) % n], 1)


def _chain(n=20000):
    v = np.arange(n - 1, dtype=np.int64)
    return n, np.stack([v, v + 1], 1)


def _two_cycles(count=2000):
    a = 2 * np.arange(count, dtype=np.int64)
    return 2 * count, np.concatenate([np.stack([a, a + 1], 1), np.stack([a + 1, a], 1),
                                      np.stack([a[:-1] + 1, a[1:]], 1)])


def _rings_in_a_chain(rings=200, size=50):
    v = np.arange(rings * size, dtype=np.int64)
    first = size * np.arange(rings - 1, dtype=np.int64)
    return rings * size, np.concatenate([np.stack([v, v - v % size + (v + 1) % size], 1),
                                         np.stack([first + 7, first + size], 1)])


def _grid_dag(side=60):
    at = np.arange(side * side, dtype=np.int64).reshape(side, side)
    across = np.stack([at[:, :-1].ravel(), at[:, 1:].ravel()], 1)
    down = np.stack([at[:-1, :].ravel(), at[1:, :].ravel()], 1)
    return side * side, np.concatenate([across, down])


def _grid_with_a_back_edge(side=60):
    n, e = _grid_dag(side)
    return n, np.concatenate([e, [(n - 1, 0)]])


def _hub(leaves=6000):
    leaf = np.arange(1, leaves + 1, dtype=np.int64)
    hub = np.zeros(leaves, np.int64)
    return leaves + 1, np.concatenate([np.stack([hub, leaf], 1), np.stack([leaf, hub], 1)])


def _random_directed(n=20000, m=30000):
    return n, np.random.default_rng(5).integers(0, n, size=(m, 2))


def _isolated_and_a_triangle():
    return 70003, np.array([(70000, 70001), (70001, 70002), (70002, 70000)], np.int64)


SHAPES = {"ring": _ring, "chain": _chain, "two_cycles": _two_cycles, "rings_in_a_chain": _rings_in_a_chain,
          "grid_dag": _grid_dag, "grid_with_a_back_edge": _grid_with_a_back_edge, "hub": _hub,
          "random_directed": _random_directed, "isolated_and_a_triangle": _isolated_and_a_triangle}


def _renumbered(name, numbering):
    n, edges = SHAPES[name]()
    edges = np.asarray(edges, np.int64)
    if numbering == "reversed":
        edges = n - 1 - edges
    if numbering == "permuted":
        edges = np.random.default_rng(9).permutation(n)[edges]
    return n, csr(n, edges, symmetric=False)


@pytest.mark.parametrize("numbering", ["as_written", "reversed", "permuted"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_that_stress_the_schedule(ea, ctx, name, numbering):
    n, (ap, aj) = _renumbered(name, numbering)
    want, count = strong_components(ap, aj)
    labels, st = check(ea, ctx, graph(ea, ap, aj).build_in_edges(ctx), want, count)
    host = labels.cpu().numpy()
    ids = np.arange(n)
    if name == "ring":
        assert count == 1 and not host.any() and st.iterations == 1
    if name == "chain":
        assert count == n and (host == ids).all() and st.iterations == 0
    if name == "two_cycles":
        # 24-25 rounds in a CPU simulation of the pivot rule in all three numberings; a balanced
        # split would need 11, one pivot at a time 2000: the cap separates those
        assert count == 2000 and st.iterations <= 64
        if numbering == "as_written":
            assert (host == ids // 2 * 2).all()
    if name == "rings_in_a_chain":
        assert count == 200
        if numbering == "as_written":
            assert (host == ids // 50 * 50).all()
    if name == "grid_dag":
        assert count == n and (host == ids).all() and st.iterations == 0
    if name == "grid_with_a_back_edge":
        assert count == 1 and not host.any() and st.iterations == 1
    if name == "hub":
        assert count == 1 and not host.any()
    if name == "random_directed":
        assert 1000 < count < n
    if name == "isolated_and_a_triangle":
        assert count == 70001 and np.bincount(host).max() == 3


@pytest.fixture(scope="module")
def hook_graphs(ea, ctx):
    """name -> (graph with in-edges, labels and count of the default run)."""
    graphs = {"rmat14": ea.Graph.rmat(ctx, 14, 16, 1, 7, symmetrize=False)}
    ap, aj, _ = known_csr("two_rings_2_to_7")
    graphs["two_rings"] = graph(ea, ap, aj)
    ap, aj, _ = known_csr("bow_tie")
    graphs["bow_tie"] = graph(ea, ap, aj)
    for name in ("hub", "two_cycles"):
        n, edges = SHAPES[name]()
        graphs[name] = graph(ea, *csr(n, edges, symmetric=False))
    out = {}
    for name, g in graphs.items():
        labels, count, _ = ea.scc(ctx, g.build_in_edges(ctx))
        out[name] = (g, labels.clone(), count)
    return out


@pytest.mark.parametrize("trim", ["0", "1"])
@pytest.mark.parametrize("narrow_edges", ["0", None])
@pytest.mark.parametrize("big_row", ["1", "1000000000"])
def test_with_the_hooks_forced(ea, ctx, monkeypatch, hook_graphs, big_row, narrow_edges, trim):
    import torch
    for name, (g, base, count) in hook_graphs.items():
        with monkeypatch.context() as m:
            m.setenv("GRX_SCC_BIG_ROW", big_row)
            m.setenv("GRX_SCC_TRIM", trim)
            if narrow_edges is not None:
                m.setenv("GRX_SCC_NARROW_EDGES", narrow_edges)
            labels, got, st = ea.scc(ctx, g)
        print(f"{name}: iterations {st.iterations} launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
        assert torch.equal(labels, base) and got == count, name
        assert st.edges_expanded == st.edges_traversed <= 2 * g.nnz * (2 * st.iterations + 2)


def test_stats(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7, symmetrize=False).build_in_edges(ctx)
    labels, count, st = ea.scc(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert st.vertices_reached == g.n_rows - count
    assert count == int((labels == torch.arange(g.n_rows, device="cuda", dtype=labels.dtype)).sum())
    assert st.edges_traversed == st.edges_expanded > 0
    assert st.advance_launches > 0 and st.iterations >= 1
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    _, _, plain = ea.scc(ctx, g)
    assert plain.advance_kernel_ms == 0 and plain.elapsed_ms > 0


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, _ = known_csr("two_rings_2_to_7")
    g = graph(ea, ap, aj)
    assert load_library().grx_scc(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.scc(ctx, graph(ea, ap, aj, n_cols=11))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.scc(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    # asymmetric and no in-edges: the call cannot walk backwards
    with pytest.raises(ea.EngineError) as e:
        ea.scc(ctx, g)
    assert e.value.code == -3
    assert b"grx_graph_build_in_edges" in load_library().grx_last_error()
    g.build_in_edges(ctx)
    with pytest.raises(TypeError):
        ea.scc(ctx, g, torch.empty(10, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.scc(ctx, g, torch.empty(9, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ea.scc(ctx, g, torch.empty(20, dtype=torch.int32, device="cuda")[::2])
    with pytest.raises(ValueError):
        ea.scc(ctx, g, torch.empty(10, dtype=torch.int32))
    # the count alone: the call works on an array of its own
    n = C.c_int64(-7)
    assert load_library().grx_scc(ctx._h, g._h, None, C.byref(n), None, None) == 0
    assert n.value == 2
    # a caller's tensor is filled in place
    mine = torch.full((10,), -1, dtype=torch.int32, device="cuda")
    out, count, _ = ea.scc(ctx, g, mine)
    assert out is mine and count == 2 and mine.cpu().tolist() == [0] * 5 + [5] * 5


def test_rmat18_invariants(ea, ctx):
    """The checker is torch and grx_bfs, not the code under test."""
    import torch
    g = ea.Graph.rmat(ctx, 18, 16, 1, 7, symmetrize=False)
    ap, aj, _ = g.to_host()
    g.build_in_edges(ctx)
    a, count, st = ea.scc(ctx, g)
    a = a.clone()
    b, count2, _ = ea.scc(ctx, g)
    assert torch.equal(a, b) and count == count2
    print(f"rmat18: components {count} iterations {st.iterations} edges_expanded {st.edges_expanded} nnz {g.nnz} "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
    la = a.long()
    n = g.n_rows
    ids = torch.arange(n, device="cuda")
    assert torch.equal(la[la], la) and bool((la <= ids).all())
    assert count == int((la == ids).sum()) and st.vertices_reached == n - count
    # the largest component is what its representative reaches, and is reached from
    giant = int(torch.bincount(la).argmax())
    unreached = torch.iinfo(torch.int32).max
    forward, _ = ea.bfs(ctx, g, giant)
    forward = forward != unreached
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    tap, taj = csr(n, np.stack([aj.astype(np.int64), src], 1), symmetric=False)
    backward, _ = ea.bfs(ctx, graph(ea, tap, taj), giant)
    assert torch.equal(forward & (backward != unreached), la == giant)
    assert int((la == giant).sum()) > 1
    # no out-entry or no in-entry besides self loops: a component of one
    proper = src != aj
    out_deg = np.bincount(src[proper], minlength=n)
    in_deg = np.bincount(aj[proper], minlength=n)
    alone = torch.from_numpy((out_deg == 0) | (in_deg == 0)).cuda()
    assert bool(alone.any()) and torch.equal(la[alone], ids[alone])
