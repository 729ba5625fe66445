"""grx_lpa (semi-synchronous label propagation over the colour classes) and grx_modularity against
the numpy oracle of tests/lpa_oracle.py, exactly: labels, count, sweeps, changes per sweep, entries
read, and I, S and Q with ==.  Known answers, chesapeake, unsorted R-MAT multigraphs with their
sorted and simple copies, shapes that stress the schedule (one row of 300 000 distinct labels,
colours beyond any small class, thousands of tiny rows), the test hooks, early stops, argument
errors and invariants on RMAT-16."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lpa_oracle import communities, csr, modularity_parts, simple_csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
HOOKS = ("GRX_LPA_LDS_SLOTS", "GRX_LPA_BIG_ROW", "GRX_LPA_NARROW_EDGES", "GRX_LPA_ALL_ROWS")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for hook in HOOKS:
        monkeypatch.delenv(hook, raising=False)


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, ap, aj, want=None, options=None, all_rows=False):
    """ea.lpa(g) equals the oracle on (ap, aj), the stats are the answer's and the score is exact."""
    want = want or communities(ap, aj)
    label, count, sweeps, changes, (decided, marked) = want
    out, n_communities, q, st = ea.lpa(ctx, g, options=options)
    assert str(out.dtype) == "torch.int32" and out.numel() == g.n_rows
    host = out.cpu().numpy()
    i, s, want_q = modularity_parts(ap, aj, label)
    print(f"V {g.n_rows} nnz {g.nnz} communities {n_communities} (oracle {count}) sweeps {st.iterations} (oracle {sweeps}) "
          f"changes {st.frontier_slots} (oracle {changes}) edges_expanded {st.edges_expanded} (oracle {decided} + {marked}) "
          f"Q {q!r} (oracle {want_q!r}) launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f} "
          f"mismatches {int((host != label).sum())}")
    assert (host == label).all()
    assert n_communities == count and st.iterations == sweeps
    assert st.frontier_slots == changes[:64]
    assert st.edges_expanded == (sweeps * g.nnz if all_rows else decided + marked)
    assert st.edges_traversed == g.nnz and st.vertices_reached == g.n_rows - count
    assert st.advance_kernel_ms == 0 and st.elapsed_ms > 0
    assert q == want_q
    assert ea.modularity(ctx, g, out) == (want_q, i, s)
    return out, st


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def _star(hub_last, leaves=300000):
    hub = leaves if hub_last else 0
    return leaves + 1, [(hub, i + (0 if hub_last else 1)) for i in range(leaves)]


def _shuffled_path():
    n = 1 << 18
    p = np.random.default_rng(3).permutation(n)
    return n, np.stack([p[:-1], p[1:]], 1)


def _grid():
    side = 300
    at = np.arange(side * side).reshape(side, side)
    return side * side, np.concatenate([np.stack([at[:, :-1].ravel(), at[:, 1:].ravel()], 1),
                                        np.stack([at[:-1].ravel(), at[1:].ravel()], 1)])


def _triangles():
    t = 3 * np.arange(50000)
    return 150000, np.concatenate([np.stack([t, t + 1], 1), np.stack([t + 1, t + 2], 1), np.stack([t + 2, t], 1)])


SHAPES = {
    "two_cliques_and_a_bridge": lambda: (10, _clique(5) + _clique(5, 5) + [(4, 5)]),
    "small_star_hub_first": lambda: _star(False, 40), "small_star_hub_last": lambda: _star(True, 40),
    "isolated_and_self_loops": lambda: (6, None),
    "no_entries": lambda: (9, []),
    "repeats_decide": lambda: (7, _clique(3) + _clique(3, 4) + [(2, 3), (3, 4), (3, 4)]),
    "star_hub_first": lambda: _star(False), "star_hub_last": lambda: _star(True),
    "k300_pendants": lambda: (1300, _clique(300) + [(i % 300, 300 + i) for i in range(1000)]),
    "shuffled_path": _shuffled_path, "grid": _grid, "triangles": _triangles,
    # 200 isolated vertices around a triangle: every class but the first holds connected vertices only
    "triangle_among_isolated": lambda: (203, [(1, 100), (100, 202), (202, 1)]),
}


@functools.lru_cache(maxsize=None)
def _shape(name):
    n, edges = SHAPES[name]()
    if edges is None:  # 0, 2 and 5 isolated, 1 with only a self loop, one edge 3-4: not symmetrised twice
        ap, aj = csr(n, np.asarray([(1, 1), (3, 4), (4, 3)], np.int64), symmetric=False)
    else:
        ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2))
    return ap, aj, communities(ap, aj)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_known_answers_and_shapes_that_stress_the_schedule(ea, ctx, name):
    ap, aj, want = _shape(name)
    out, st = check(ea, ctx, graph(ea, ap, aj), ap, aj, want)
    c = out.cpu().numpy()
    if name == "two_cliques_and_a_bridge":
        assert c.tolist() == [0] * 5 + [5] * 5 and st.iterations == 2 and g_parts(ap, aj, c) == (40, 882)
        assert ea.modularity(ctx, graph(ea, ap, aj), out)[0] == 40 / 42 - 0.5
    if "star" in name:
        assert (c == 0).all() and st.iterations == 2
    if name == "isolated_and_self_loops":
        assert c.tolist() == [0, 1, 2, 3, 3, 5]
    if name == "no_entries":
        assert c.tolist() == list(range(9)) and st.iterations == 1 and st.edges_expanded == 0
    if name == "repeats_decide":
        assert c[3] == c[4] and c[3] != c[2]
    if name == "triangle_among_isolated":
        assert want[1] == 201 and st.iterations == 2 and (c[[1, 100, 202]] == 1).all()
    if name == "triangles":
        assert (c.reshape(-1, 3) == c.reshape(-1, 3)[:, :1]).all() and (c[::3] == np.arange(0, 150000, 3)).all()


def g_parts(ap, aj, label):
    return modularity_parts(ap, aj, label)[:2]


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    check(ea, ctx, g, ap, aj[: g.nnz])


_RMAT = {}


def _rmat(ea, ctx, scale):
    """(ap, aj, oracle answer) of the symmetric R-MAT multigraph as generated; computed once."""
    if scale not in _RMAT:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, _ = g.to_host()
        aj = aj[: g.nnz]
        _RMAT[scale] = (ap, aj, communities(ap, aj))
    return _RMAT[scale]


@pytest.mark.parametrize("scale", [12, 14])
def test_rmat_multigraph_sorted_and_simple(ea, ctx, scale):
    import torch
    ap, aj, want = _rmat(ea, ctx, scale)
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    out, st = check(ea, ctx, g, ap, aj, want)
    out = out.clone()
    # the same rows in another order: the same answer
    o2, n2, q2, st2 = ea.lpa(ctx, g.sorted_rows(ctx))
    assert torch.equal(o2, out) and n2 == want[1] and st2.iterations == st.iterations
    assert st2.frontier_slots == st.frontier_slots and st2.edges_expanded == st.edges_expanded
    assert q2 == modularity_parts(ap, aj, want[0])[2]
    # the simple graph counts every neighbour once: its own oracle run
    sap, saj = simple_csr(ap, aj)
    s = g.simple(ctx)
    assert s.nnz == len(saj)
    check(ea, ctx, s, sap, saj)


def _hooked_graph(ea, ctx, name):
    if name == "rmat12":
        return ea.Graph.rmat(ctx, 12, 16, 1, 7), _rmat(ea, ctx, 12)
    ap, aj, want = _shape(name)
    return graph(ea, ap, aj), (ap, aj, want)


@pytest.mark.parametrize("hook,value", [("GRX_LPA_LDS_SLOTS", "64"), ("GRX_LPA_BIG_ROW", "8"),
                                        ("GRX_LPA_NARROW_EDGES", "0"), ("GRX_LPA_ALL_ROWS", "1")])
@pytest.mark.parametrize("name", ["rmat12", "star_hub_first"])
def test_with_the_thresholds_forced(ea, ctx, monkeypatch, name, hook, value):
    import torch
    g, (ap, aj, want) = _hooked_graph(ea, ctx, name)
    base, _ = check(ea, ctx, g, ap, aj, want)
    base = base.clone()
    monkeypatch.setenv(hook, value)
    out, _ = check(ea, ctx, g, ap, aj, want, all_rows=hook == "GRX_LPA_ALL_ROWS")
    assert torch.equal(out, base)
    monkeypatch.delenv(hook)


def test_two_hooks_at_once_send_every_long_row_through_the_global_table(ea, ctx, monkeypatch):
    ap, aj, want = _rmat(ea, ctx, 12)
    g = ea.Graph.rmat(ctx, 12, 16, 1, 7)
    monkeypatch.setenv("GRX_LPA_LDS_SLOTS", "64")
    monkeypatch.setenv("GRX_LPA_BIG_ROW", "8")
    check(ea, ctx, g, ap, aj, want)
    monkeypatch.setenv("GRX_LPA_NARROW_EDGES", "0")
    check(ea, ctx, g, ap, aj, want)


@pytest.mark.parametrize("sweeps", [1, 2])
def test_early_stop_is_a_prefix(ea, ctx, sweeps):
    ap, aj, full = _rmat(ea, ctx, 12)
    assert full[2] > 2
    g = ea.Graph.rmat(ctx, 12, 16, 1, 7)
    want = communities(ap, aj, max_sweeps=sweeps)
    assert want[3] == full[3][:sweeps]
    check(ea, ctx, g, ap, aj, want, options=ea.Options(max_iterations=sweeps))


def test_modularity_alone_and_of_other_labellings(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, want = _rmat(ea, ctx, 12)
    g = ea.Graph.rmat(ctx, 12, 16, 1, 7)
    i, s, want_q = modularity_parts(ap, aj, want[0])
    # the score alone: the call works on an array of its own
    q = C.c_double(-7.0)
    assert load_library().grx_lpa(ctx._h, g._h, None, None, C.byref(q), None, None) == 0
    assert q.value == want_q
    n = C.c_int64(-7)
    assert load_library().grx_lpa(ctx._h, g._h, None, C.byref(n), None, None, None) == 0
    assert n.value == want[1]
    # a caller's tensor is filled in place
    mine = torch.full((g.n_rows,), -5, dtype=torch.int32, device="cuda")
    out, count, q2, _ = ea.lpa(ctx, g, mine)
    assert out is mine and count == want[1] and q2 == want_q and (mine.cpu().numpy() == want[0]).all()
    # the components, and everything in one community: I = E and S = E^2, so Q = 0.0 exactly
    comp, _, _ = ea.cc(ctx, g)
    ci, cs, cq = modularity_parts(ap, aj, comp.cpu().numpy())
    assert ea.modularity(ctx, g, comp) == (cq, ci, cs)
    zero = torch.zeros(g.n_rows, dtype=torch.int32, device="cuda")
    assert ea.modularity(ctx, g, zero) == (0.0, g.nnz, g.nnz * g.nnz)
    # each output alone, and stats
    st = ea.api._Stats()
    inside = C.c_int64(-1)
    assert load_library().grx_modularity(ctx._h, g._h, out.data_ptr(), None, C.byref(inside), None, None,
                                         C.byref(st)) == 0
    assert inside.value == i and st.iterations == 1 and st.edges_traversed == st.edges_expanded == g.nnz
    assert st.advance_launches > 0 and st.elapsed_ms > 0
    # a directed CSR is accepted: every entry counts as given
    d = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    dap, daj, _ = d.to_host()
    label = (np.arange(d.n_rows) % 5).astype(np.int32)
    di, ds, dq = modularity_parts(dap, daj[: d.nnz], label)
    assert ea.modularity(ctx, d, torch.from_numpy(label).cuda()) == (dq, di, ds)


def test_stats_with_kernel_time(ea, ctx):
    ap, aj, want = _rmat(ea, ctx, 14)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    _, _, _, st = ea.lpa(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    assert st.frontier_slots == want[3][:64] and st.iterations == want[2]  # change counts, never microseconds


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, _ = _shape("two_cliques_and_a_bridge")
    g = graph(ea, ap, aj)
    lib = load_library()
    assert lib.grx_lpa(ctx._h, g._h, None, None, None, None, None) == -1
    assert lib.grx_lpa(None, g._h, None, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.lpa(ctx, graph(ea, ap, aj, n_cols=11))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.lpa(ctx, g, options=ea.Options(max_iterations=-1))
    assert e.value.code == -1
    with pytest.raises(TypeError):
        ea.lpa(ctx, g, torch.empty(10, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.lpa(ctx, g, torch.empty(9, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ea.lpa(ctx, g, torch.empty(10, dtype=torch.int32))
    # grx_modularity: no output, a non-square graph, labels outside [0, V)
    label = torch.zeros(10, dtype=torch.int32, device="cuda")
    assert lib.grx_modularity(ctx._h, g._h, label.data_ptr(), None, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.modularity(ctx, graph(ea, ap, aj, n_cols=11), label)
    assert e.value.code == -1
    for bad in (10, -1):
        label = torch.zeros(10, dtype=torch.int32, device="cuda")
        label[7] = bad
        with pytest.raises(ea.EngineError) as e:
            ea.modularity(ctx, g, label)
        assert e.value.code == -1
    with pytest.raises(TypeError):
        ea.modularity(ctx, g, torch.zeros(10, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.modularity(ctx, g, torch.zeros(11, dtype=torch.int32, device="cuda"))


def test_directed_input_is_unsupported(ea, ctx):
    with pytest.raises(ea.EngineError) as e:
        ea.lpa(ctx, ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False))
    assert e.value.code == -3
    ap, aj, _ = _shape("two_cliques_and_a_bridge")
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.lpa(ctx, g)
    assert e.value.code == -3


def test_the_empty_graph(ea, ctx):
    g = graph(ea, np.zeros(1, np.int32), np.zeros(0, np.int32))
    out, count, q, st = ea.lpa(ctx, g)
    assert out.numel() == 0 and count == 0 and q == 0.0 and st.iterations == 0
    assert ea.modularity(ctx, g, out) == (0.0, 0, 0)


def test_rmat16_invariants(ea, ctx):
    """The checker is numpy on the host, not the code under test."""
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    a, count, q, st = ea.lpa(ctx, g)
    a = a.clone()
    b, count2, q2, st2 = ea.lpa(ctx, g)
    assert torch.equal(a, b) and (count, q, st.iterations, st.frontier_slots, st.edges_expanded) == \
        (count2, q2, st2.iterations, st2.frontier_slots, st2.edges_expanded)
    print(f"RMAT-16: communities {count} Q {q:.4f} sweeps {st.iterations} changes {st.frontier_slots} "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}")
    ap, aj, _ = g.to_host()
    ap = ap.astype(np.int64)
    aj = aj[: g.nnz].astype(np.int64)
    n = g.n_rows
    label = a.cpu().numpy().astype(np.int64)
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    assert count == int((label == np.arange(n)).sum()) and st.vertices_reached == n - count
    assert st.frontier_slots[-1] == 0 and all(c > 0 for c in st.frontier_slots[:-1])
    # the run stopped: every vertex's label is among the most frequent of its row
    row = np.repeat(np.arange(n), np.diff(ap))
    keep = row != aj
    pair, cnt = np.unique(row[keep] * n + label[aj[keep]], return_counts=True)
    v, l = pair // n, pair % n
    best = np.zeros(n, np.int64)
    np.maximum.at(best, v, cnt)
    own = np.zeros(n, np.int64)
    mine = l == label[v]
    own[v[mine]] = cnt[mine]
    assert (own == best).all()
    assert q == modularity_parts(ap, aj, label)[2]
