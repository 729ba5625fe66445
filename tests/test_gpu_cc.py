"""grx_cc (connected components; weakly connected on a directed CSR) against the numpy oracle of
tests/cc_oracle.py, exactly: known answers, chesapeake, symmetric and directed R-MAT in several
layouts, shapes that stress the schedule (deep parent chains, one contended root, no giant
component), the test hooks, the stats, argument errors and invariants on RMAT-22.  The label of a
vertex is the smallest vertex id of its component; edges_expanded == nnz unless the handle is known
to be symmetric, and at most nnz / 8 on the symmetric R-MAT as generated."""
import ctypes as C
import os

import numpy as np
import pytest

from cc_oracle import KNOWN, components, csr, known_csr

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


def check(ea, ctx, g, want, count, full_walk=None, options=None):
    """ea.cc(g) gives `want` exactly; the stats are the answer's.  full_walk: True = every entry is
    read, False = fewer, None = either."""
    labels, got, st = ea.cc(ctx, g, options=options)
    assert str(labels.dtype) == "torch.int32" and labels.numel() == g.n_rows
    host = labels.cpu().numpy()
    assert (host == want).all()
    assert got == count == int((host == np.arange(g.n_rows)).sum())
    assert st.vertices_reached == g.n_rows - count
    assert st.edges_expanded == st.edges_traversed and 0 <= st.edges_expanded <= g.nnz
    if g.nnz:
        assert st.edges_expanded > 0
    if g.n_rows:
        assert st.advance_launches > 0 and st.iterations >= 1
    if full_walk is True:
        assert st.edges_expanded == g.nnz
    if full_walk is False:
        assert st.edges_expanded < g.nnz
    print(f"V {g.n_rows} nnz {g.nnz} components {got} edges_expanded {st.edges_expanded} "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
    return labels, st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, want = known_csr(name)
    labels, _ = check(ea, ctx, graph(ea, ap, aj), *components(ap, aj), full_walk=True)
    assert labels.cpu().numpy().tolist() == want.tolist()


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    labels, _ = check(ea, ctx, g, *components(ap, aj))
    assert g.n_rows == 39 and not labels.cpu().numpy().any()


@pytest.mark.parametrize("scale", [16, 18, 20])
def test_symmetric_rmat_in_every_layout(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    ap, aj, ax = g.to_host()
    want, count = components(ap, aj)
    labels, _ = check(ea, ctx, g, want, count, full_walk=False)
    for other in (g.sorted_rows(ctx), g.simple(ctx)):
        check(ea, ctx, other, want, count)
    if scale == 16:
        # the same arrays as a non-owning view: nobody knows that it is symmetric, and grx_cc does
        # not find out, so every row is walked -- on the second call too
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ap, aj, ax)]
        view = ea.Graph.from_device_csr(*dev)
        check(ea, ctx, view, want, count, full_walk=True)
        check(ea, ctx, view, want, count, full_walk=True)
        ea.kcore(ctx, view)  # verifies the symmetry and leaves the verdict on the handle
        again, _ = check(ea, ctx, view, want, count, full_walk=False)
        assert torch.equal(again, labels)


@pytest.mark.parametrize("scale", [16, 18])
def test_directed_rmat_weak_components(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=False)
    ap, aj, _ = g.to_host()
    want, count = components(ap, aj)
    labels, _ = check(ea, ctx, g, want, count, full_walk=True)
    labels = labels.clone()
    g.build_in_edges(ctx)
    again, _ = check(ea, ctx, g, want, count, full_walk=True)
    assert torch.equal(again, labels)


def _path(n=1 << 20):
    v = np.arange(n - 1, dtype=np.int64)
    return n, np.stack([v, v + 1], 1)


def _shuffled_path():
    n, e = _path()
    return n, np.random.default_rng(3).permutation(n)[e]


def _star_hub_first(leaves=300000):
    return leaves + 1, np.stack([np.zeros(leaves, np.int64), np.arange(1, leaves + 1)], 1)


def _star_hub_last(leaves=300000):
    return leaves + 1, np.stack([np.full(leaves, leaves, np.int64), np.arange(leaves)], 1)


def _grid(side=300):
    at = np.arange(side * side, dtype=np.int64).reshape(side, side)
    across = np.stack([at[:, :-1].ravel(), at[:, 1:].ravel()], 1)
    down = np.stack([at[:-1, :].ravel(), at[1:, :].ravel()], 1)
    return side * side, np.concatenate([across, down])


def _triangles(count=100000):
    a = 3 * np.arange(count, dtype=np.int64)
    return 3 * count, np.concatenate([np.stack([a, a + 1], 1), np.stack([a + 1, a + 2], 1), np.stack([a + 2, a], 1)])


def _rings(rings=1000, size=1000):
    v = np.arange(rings * size, dtype=np.int64)
    return rings * size, np.stack([v, v - v % size + (v + 1) % size], 1)


def _isolated_and_a_triangle():
    return 70003, np.array([(70000, 70001), (70001, 70002), (70002, 70000)], np.int64)


SHAPES = {"path": _path, "shuffled_path": _shuffled_path, "star_hub_first": _star_hub_first,
          "star_hub_last": _star_hub_last, "grid": _grid, "triangles": _triangles, "rings": _rings,
          "isolated_and_a_triangle": _isolated_and_a_triangle}


@pytest.mark.parametrize("verified", [False, True])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_that_stress_the_schedule(ea, ctx, name, verified):
    """verified: a triangle count has left the verdict "symmetric" on the handle first, so the rows
    of the picked component stay unread; otherwise every row is walked."""
    n, edges = SHAPES[name]()
    ap, aj = csr(n, edges)
    g = graph(ea, ap, aj)
    if verified:
        ea.tc(ctx, g, per_vertex=False)
    want, count = components(ap, aj)
    labels, st = check(ea, ctx, g, want, count, full_walk=None if verified else True)
    host = labels.cpu().numpy()
    if name in ("path", "shuffled_path", "star_hub_first", "star_hub_last", "grid"):
        assert count == 1 and not host.any()
    if name == "triangles":
        assert count == 100000 and (host == np.arange(n) // 3 * 3).all()
    if name == "rings":
        assert count == 1000 and (host == np.arange(n) // 1000 * 1000).all()
    if name == "isolated_and_a_triangle":
        assert count == 70001 and (host[:70000] == np.arange(70000)).all() and (host[70000:] == 70000).all()


def _hook_graphs(ea, ctx):
    yield "rmat16", ea.Graph.rmat(ctx, 16, 16, 1, 7)
    for name in ("star_hub_first", "star_hub_last"):
        n, edges = SHAPES[name]()
        yield name, graph(ea, *csr(n, edges))
    n, edges = SHAPES["star_hub_last"]()
    g = graph(ea, *csr(n, edges))
    ea.tc(ctx, g, per_vertex=False)  # verifies the symmetry: the verdict stays on the handle
    yield "star_hub_last_verified", g


@pytest.mark.parametrize("big_row", ["1", "1000000000"])
@pytest.mark.parametrize("rounds", ["0", "1", "2", "5"])
def test_with_the_hooks_forced(ea, ctx, monkeypatch, rounds, big_row):
    import torch
    for name, g in _hook_graphs(ea, ctx):
        base, count, _ = ea.cc(ctx, g)
        base = base.clone()
        with monkeypatch.context() as m:
            m.setenv("GRX_CC_SAMPLE_ROUNDS", rounds)
            m.setenv("GRX_CC_BIG_ROW", big_row)
            labels, got, st = ea.cc(ctx, g)
        assert torch.equal(labels, base) and got == count, name
        assert st.iterations == int(rounds) + 1
        assert 0 < st.edges_expanded <= g.nnz
        if rounds == "0" or not name.startswith("rmat") and not name.endswith("verified"):
            assert st.edges_expanded == g.nnz, name


def test_stats(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 18, 16, 1, 7)
    labels, count, st = ea.cc(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert st.vertices_reached == g.n_rows - count
    assert count == int((labels == torch.arange(g.n_rows, device="cuda", dtype=labels.dtype)).sum())
    assert 0 < st.edges_expanded <= g.nnz and st.edges_traversed == st.edges_expanded
    assert st.advance_launches > 0 and st.iterations == 3
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    _, _, plain = ea.cc(ctx, g)
    assert plain.advance_kernel_ms == 0 and plain.elapsed_ms > 0


@pytest.mark.parametrize("scale", [16, 18, 20, 22])
def test_the_skip_is_real(ea, ctx, scale):
    """Two neighbour rounds leave nearly the whole giant component under one root, and its rows are
    not read: a CPU simulation of the rounds on an R-MAT of these parameters read 0.034 - 0.037 of
    nnz, the bound leaves a factor of three."""
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    _, count, st = ea.cc(ctx, g)
    print(f"rmat{scale}: V {g.n_rows} nnz {g.nnz} components {count} edges_expanded {st.edges_expanded} "
          f"ratio {st.edges_expanded / g.nnz:.4f} elapsed_ms {st.elapsed_ms:.3f}")
    assert 0 < st.edges_expanded <= g.nnz / 8


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, _ = known_csr("two_cliques")
    g = graph(ea, ap, aj)
    assert load_library().grx_cc(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.cc(ctx, graph(ea, ap, aj, n_cols=10))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.cc(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    with pytest.raises(TypeError):
        ea.cc(ctx, g, torch.empty(9, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.cc(ctx, g, torch.empty(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ea.cc(ctx, g, torch.empty(18, dtype=torch.int32, device="cuda")[::2])
    with pytest.raises(ValueError):
        ea.cc(ctx, g, torch.empty(9, dtype=torch.int32))
    # the count alone: the call works on an array of its own
    n = C.c_int64(-7)
    assert load_library().grx_cc(ctx._h, g._h, None, C.byref(n), None, None) == 0
    assert n.value == 2
    # a caller's tensor is filled in place
    mine = torch.full((9,), -1, dtype=torch.int32, device="cuda")
    out, count, _ = ea.cc(ctx, g, mine)
    assert out is mine and count == 2 and mine.cpu().tolist() == [0] * 4 + [4] * 5


def test_rmat22_invariants(ea, ctx):
    """The checker is torch and grx_bfs, not the code under test."""
    import torch
    g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
    a, count, st = ea.cc(ctx, g, options=ea.Options(collect_kernel_time=True))
    a = a.clone()
    b, count2, _ = ea.cc(ctx, g)
    assert torch.equal(a, b) and count == count2
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    la = a.long()
    ids = torch.arange(g.n_rows, device="cuda")
    assert torch.equal(la[la], la) and bool((la <= ids).all())
    assert count == int((la == ids).sum()) and st.vertices_reached == g.n_rows - count
    ap, aj, _ = g.to_host()
    off = torch.from_numpy(ap.astype(np.int64)).cuda()
    row = torch.repeat_interleave(ids, off[1:] - off[:-1])
    col = torch.from_numpy(aj.astype(np.int64)).cuda()
    assert torch.equal(la[row], la[col])
    del row, col
    # the largest component is exactly what a BFS from its representative reaches
    giant = int(torch.bincount(la).argmax())
    depth, _ = ea.bfs(ctx, g, giant)
    assert torch.equal(depth != torch.iinfo(torch.int32).max, la == giant)
    want, n_want = components(ap, aj)
    assert n_want == count and (a.cpu().numpy() == want).all()
    g.hot_first(ctx, True)
    c, count3, _ = ea.cc(ctx, g)
    assert torch.equal(c, a) and count3 == count
