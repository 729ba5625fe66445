"""grx_mst (minimum spanning forest of the CSR as given) against the numpy oracle of
tests/mst_oracle.py, exactly -- entries, count, float(weight) and labels: known answers, chesapeake
(ties alone), weighted and unit-weight R-MAT in several layouts, directed R-MAT, shapes that stress
the schedule (hooking chains a million long, one contended root, no giant component), the test
hooks, the stats, argument errors, and invariants on RMAT-22 checked with torch and grx_cc.  Every
check also asserts count == V - components, labels == ea.cc on the same handle, entries strictly
ascending and no chosen self loop."""
import ctypes as C
import os

import numpy as np
import pytest

from mst_oracle import KNOWN, forest, known_csr, weighted_csr

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


def rounds_bound(n):
    """ceil(log2 V) + 1"""
    return (max(n, 1) - 1).bit_length() + 1


def check(ea, ctx, g, options=None):
    """ea.mst(g) is the oracle's forest of g's own host arrays, exactly.  Returns (entries, weight,
    labels, stats) with the tensors cloned."""
    import torch
    ap, aj, ax = g.to_host()
    want_entries, want_weight, want_labels = forest(ap, aj, ax)
    entries, weight, labels, st = ea.mst(ctx, g, components=True, options=options)
    assert str(entries.dtype) == "torch.int32" and str(labels.dtype) == "torch.int32"
    assert labels.numel() == g.n_rows and isinstance(weight, float)
    host = entries.cpu().numpy()
    print(f"V {g.n_rows} nnz {g.nnz} count {len(host)} weight {weight!r} want {want_weight!r} rounds {st.iterations} "
          f"edges_expanded {st.edges_expanded} launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
    assert host.tolist() == want_entries.tolist()
    assert weight == want_weight
    assert (labels.cpu().numpy() == want_labels).all()
    cc_labels, components, _ = ea.cc(ctx, g)
    assert torch.equal(labels, cc_labels)
    assert len(host) == g.n_rows - components == st.vertices_reached
    assert (np.diff(host) > 0).all()
    src = np.repeat(np.arange(g.n_rows), np.diff(ap))
    assert (src[host] != aj[host]).all()
    assert st.edges_expanded == st.edges_traversed
    assert 0 <= st.iterations <= rounds_bound(g.n_rows)
    if g.nnz:
        assert g.nnz <= st.edges_expanded <= st.iterations * g.nnz and st.advance_launches > 0
    return entries.clone(), weight, labels.clone(), st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, ax, want, weight = known_csr(name)
    entries, got, _, _ = check(ea, ctx, ea.Graph.from_host_csr(ap, aj, ax))
    assert entries.cpu().numpy().tolist() == want.tolist() and got == weight


def test_chesapeake(ea, ctx):
    """Every weight is equal: positions alone decide."""
    g = ea.Graph.from_mtx(CHESAPEAKE)
    assert (g.to_host()[2] == g.to_host()[2][0]).all()
    entries, _, labels, _ = check(ea, ctx, g)
    assert g.n_rows == 39 and entries.numel() == 38 and not labels.cpu().numpy().any()


@pytest.mark.parametrize("scale", [16, 18, 20])
def test_symmetric_rmat_in_every_layout(ea, ctx, scale):
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    _, weight, labels, _ = check(ea, ctx, g)
    for other in (g.sorted_rows(ctx), g.simple(ctx)):
        _, w, l, _ = check(ea, ctx, other)
        assert w == weight and (l == labels).all()


def test_unit_weight_rmat(ea, ctx):
    g = ea.Graph.rmat(ctx, 16, 16, 1, 0)
    assert (g.to_host()[2] == 1).all()
    entries, weight, _, _ = check(ea, ctx, g)
    assert weight == float(entries.numel())


@pytest.mark.parametrize("scale", [16, 18])
def test_directed_rmat(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=False)
    entries, weight, labels, _ = check(ea, ctx, g)
    g.build_in_edges(ctx)
    again, w, l, _ = check(ea, ctx, g)
    assert torch.equal(again, entries) and w == weight and torch.equal(l, labels)


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
COUNTS = {"path": (1 << 20) - 1, "shuffled_path": (1 << 20) - 1, "star_hub_first": 300000, "star_hub_last": 300000,
          "grid": 300 * 300 - 1, "triangles": 200000, "rings": 999000, "isolated_and_a_triangle": 2}


def shape_graph(ea, name, equal):
    n, edges = SHAPES[name]()
    weights = np.ones(len(edges)) if equal else np.random.default_rng(5).integers(1, 5, len(edges))
    return ea.Graph.from_host_csr(*weighted_csr(n, edges, weights))


@pytest.mark.parametrize("equal", [False, True])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_that_stress_the_schedule(ea, ctx, name, equal):
    g = shape_graph(ea, name, equal)
    entries, weight, _, st = check(ea, ctx, g)
    assert entries.numel() == COUNTS[name]
    if equal:
        assert weight == float(COUNTS[name])
    if name in ("path", "shuffled_path"):
        assert st.iterations <= 21


def _hook_graphs(ea, ctx):
    yield "rmat16", ea.Graph.rmat(ctx, 16, 16, 1, 7)
    for name in ("star_hub_first", "star_hub_last"):
        yield name, shape_graph(ea, name, False)


@pytest.mark.parametrize("flags", ["0", "1"])
@pytest.mark.parametrize("big_row", ["1", "1000000000"])
def test_with_the_hooks_forced(ea, ctx, monkeypatch, big_row, flags):
    import torch
    for name, g in _hook_graphs(ea, ctx):
        base = ea.mst(ctx, g, components=True)
        entries, labels = base[0].clone(), base[2].clone()
        with monkeypatch.context() as m:
            m.setenv("GRX_MST_BIG_ROW", big_row)
            m.setenv("GRX_MST_ROW_FLAGS", flags)
            got = ea.mst(ctx, g, components=True)
        assert torch.equal(got[0], entries) and got[1] == base[1] and torch.equal(got[2], labels), name
        st = got[3]
        assert st.iterations == base[3].iterations <= rounds_bound(g.n_rows), name
        assert g.nnz <= st.edges_expanded <= st.iterations * g.nnz, name
        if flags == "0":  # every row in every round
            assert st.edges_expanded == st.iterations * g.nnz, name


def test_stats(ea, ctx):
    g = ea.Graph.rmat(ctx, 18, 16, 1, 7)
    entries, _, _, st = ea.mst(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert st.vertices_reached == entries.numel()
    assert g.nnz <= st.edges_expanded <= st.iterations * g.nnz and st.edges_traversed == st.edges_expanded
    assert st.advance_launches > 0 and 1 <= st.iterations <= rounds_bound(g.n_rows)
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    _, _, _, plain = ea.mst(ctx, g)
    assert plain.advance_kernel_ms == 0 and plain.elapsed_ms > 0
    assert plain.iterations == st.iterations and plain.edges_expanded == st.edges_expanded


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, ax, want, weight = known_csr("two_cliques_bridge")
    g = ea.Graph.from_host_csr(ap, aj, ax)
    lib = load_library()
    assert lib.grx_mst(ctx._h, g._h, None, None, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.mst(ctx, ea.Graph.from_host_csr(ap, aj, ax, n_cols=10))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.mst(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    for kind in ("entries", "components"):
        with pytest.raises(TypeError):
            ea.mst(ctx, g, **{kind: torch.empty(6, dtype=torch.int64, device="cuda")})
        with pytest.raises(ValueError):
            ea.mst(ctx, g, **{kind: torch.empty(5, dtype=torch.int32, device="cuda")})
        with pytest.raises(ValueError):
            ea.mst(ctx, g, **{kind: torch.empty(12, dtype=torch.int32, device="cuda")[::2]})
        with pytest.raises(ValueError):
            ea.mst(ctx, g, **{kind: torch.empty(6, dtype=torch.int32)})
    # the weight alone, the count alone: the call works on arrays of its own
    w = C.c_double(-7.0)
    assert lib.grx_mst(ctx._h, g._h, None, None, C.byref(w), None, None, None) == 0
    assert w.value == weight
    n = C.c_int64(-7)
    assert lib.grx_mst(ctx._h, g._h, None, C.byref(n), None, None, None, None) == 0
    assert n.value == len(want)
    # the caller's tensors are filled in place; the labels come back as the same object, the entries
    # as the leading slice of theirs
    mine = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    labels = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    out, got, same, _ = ea.mst(ctx, g, mine, labels)
    assert same is labels and labels.cpu().tolist() == [0] * 6
    assert out.data_ptr() == mine.data_ptr() and got == weight
    assert mine.cpu().tolist() == want.tolist() + [-1]
    # no labels unless asked for
    assert ea.mst(ctx, g)[2] is None
    # the empty graph
    empty = ea.Graph.from_host_csr(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    n, w = C.c_int64(-7), C.c_double(-7.0)
    assert lib.grx_mst(ctx._h, empty._h, None, C.byref(n), C.byref(w), None, None, None) == 0
    assert n.value == 0 and w.value == 0.0


def test_rmat22_invariants(ea, ctx):
    """The checker is torch and grx_cc, not the code under test, and not the oracle: exactness
    against mst_oracle.forest is pinned at scales <= 20 (the tests above); at scale 22 the oracle is
    not run.  What is checked here: two calls are bit-identical; the chosen entries' subgraph has
    the whole graph's components and count == V - components, which together make it a spanning
    forest; the weight is the float64 sum of the chosen weights; and the weight is that of the
    sorted-rows layout, of the simple graph and of the same handle with a hot-first copy built."""
    import torch
    g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
    a = ea.mst(ctx, g, components=True, options=ea.Options(collect_kernel_time=True))
    entries, weight, labels, st = a[0].clone(), a[1], a[2].clone(), a[3]
    b = ea.mst(ctx, g, components=True)
    assert torch.equal(b[0], entries) and b[1] == weight and torch.equal(b[2], labels)
    assert b[3].iterations == st.iterations <= rounds_bound(g.n_rows)
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    print(f"rmat22: V {g.n_rows} nnz {g.nnz} count {entries.numel()} weight {weight!r} rounds {st.iterations} "
          f"edges_expanded {st.edges_expanded} ({st.edges_expanded / g.nnz:.3f} nnz) elapsed_ms {st.elapsed_ms:.3f} "
          f"kernel_ms {st.advance_kernel_ms:.3f}")
    cc_labels, components, _ = ea.cc(ctx, g)
    assert torch.equal(labels, cc_labels) and entries.numel() == g.n_rows - components == st.vertices_reached
    ap, aj, ax = g.to_host()
    at = entries.long()
    assert bool((at[1:] > at[:-1]).all())
    off = torch.from_numpy(ap.astype(np.int64)).cuda()
    col = torch.from_numpy(aj).cuda()
    val = torch.from_numpy(ax).cuda()
    row = (torch.searchsorted(off, at, right=True) - 1).int()
    assert bool((off[row.long()] <= at).all()) and bool((at < off[row.long() + 1]).all())
    picked = col[at]
    assert bool((row != picked).all())
    assert weight == float(val[at].double().sum())
    # the forest alone, as a directed CSR of V rows (entries ascend, so rows do too)
    tree_off = torch.zeros(g.n_rows + 1, dtype=torch.int64, device="cuda")
    tree_off[1:] = torch.cumsum(torch.bincount(row.long(), minlength=g.n_rows), 0)
    tree = ea.Graph.from_device_csr(tree_off.int(), picked.contiguous(), val[at].contiguous())
    tree_labels, tree_components, _ = ea.cc(ctx, tree)
    assert tree_components == components and torch.equal(tree_labels, cc_labels)
    del tree, off, col, val
    for other in (g.sorted_rows(ctx), g.simple(ctx)):
        got = ea.mst(ctx, other)
        assert got[1] == weight and got[0].numel() == entries.numel()
    g.hot_first(ctx, True)
    c = ea.mst(ctx, g, components=True)
    assert torch.equal(c[0], entries) and c[1] == weight and torch.equal(c[2], labels)
