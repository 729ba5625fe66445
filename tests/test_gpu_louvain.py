"""grx_louvain (multi-level modularity optimisation in exact integers) against the numpy oracle of
tests/louvain_oracle.py, exactly: labels, count, levels, sweeps, moves kept per sweep, entries
expanded and Q with ==, and grx_modularity of the result.  Known answers (the undo case and the
planted partition among them), chesapeake, an unsorted R-MAT multigraph with its sorted and simple
copies, shapes that stress the schedule (one row above every LDS table, many equal gains, thousands
of tiny rows, many levels, a weighted big row on a coarse level), the test hooks, dendrogram cuts,
repeat calls, NULL outputs, argument errors and invariants on RMAT-16."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from louvain_oracle import UNDO_EDGES, communities, csr, level_graph, modularity_parts, planted, simple_csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
HOOKS = ("GRX_LOUVAIN_LDS_SLOTS", "GRX_LOUVAIN_BIG_ROW", "GRX_LOUVAIN_NARROW_EDGES")


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


def check(ea, ctx, g, ap, aj, want=None, options=None):
    """ea.louvain(g) equals the oracle on (ap, aj), the stats are the answer's and the score is exact."""
    want = want or communities(ap, aj)
    label, count, want_q, levels, kept, shapes = want
    out, n_communities, q, n_levels, st = ea.louvain(ctx, g, options=options)
    assert str(out.dtype) == "torch.int32" and out.numel() == g.n_rows
    host = out.cpu().numpy()
    # every sweep of phase p walks that level graph's entries
    expanded, phase = 0, 0
    for moved in kept:
        expanded += shapes[phase][1]
        phase += moved == 0
    print(f"V {g.n_rows} nnz {g.nnz} communities {n_communities} (oracle {count}) levels {n_levels} (oracle {levels}) "
          f"sweeps {st.iterations} (oracle {len(kept)}) kept {st.frontier_slots} (oracle {kept}) level graphs {shapes} "
          f"edges_expanded {st.edges_expanded} (oracle {expanded}) Q {q!r} (oracle {want_q!r}) "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f} mismatches {int((host != label).sum())}")
    assert (host == label).all()
    assert n_communities == count and n_levels == levels and st.iterations == len(kept)
    assert st.frontier_slots == kept[:64] and st.edges_expanded == expanded
    assert st.edges_traversed == g.nnz and st.vertices_reached == g.n_rows - count
    assert st.advance_kernel_ms == 0 and st.elapsed_ms > 0
    assert q == want_q
    assert ea.modularity(ctx, g, out)[0] == q
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


def _hub_of_cliques():
    """Vertex 0 joined to one vertex of each of 100 K5: on level 1 its community has 100 entries."""
    edges = []
    for i in range(100):
        edges += _clique(5, 1 + 5 * i) + [(0, 1 + 5 * i)]
    return 501, edges


SHAPES = {
    "two_cliques_and_a_bridge": lambda: (10, _clique(5) + _clique(5, 5) + [(4, 5)]),
    "undo": lambda: (8, UNDO_EDGES),
    "isolated_and_self_loops": lambda: (6, None),
    "no_entries": lambda: (9, []),
    "star_hub_first": lambda: _star(False), "star_hub_last": lambda: _star(True),
    "k300_pendants": lambda: (1300, _clique(300) + [(i % 300, 300 + i) for i in range(1000)]),
    "shuffled_path": _shuffled_path, "grid": _grid, "triangles": _triangles,
    "hub_of_cliques": _hub_of_cliques,
    # 200 isolated vertices around a triangle: every class but the first holds connected vertices only
    "triangle_among_isolated": lambda: (203, [(1, 100), (100, 202), (202, 1)]),
}


@functools.lru_cache(maxsize=None)
def _shape(name):
    if name == "planted":
        ap, aj, _ = planted()
        return ap, aj, communities(ap, aj)
    n, edges = SHAPES[name]()
    if edges is None:  # 0, 2 and 5 isolated, 1 with only a self loop, one edge 3-4: not symmetrised twice
        ap, aj = csr(n, np.asarray([(1, 1), (3, 4), (4, 3)], np.int64), symmetric=False)
    else:
        ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2))
    return ap, aj, communities(ap, aj)


@pytest.mark.parametrize("name", sorted(SHAPES) + ["planted"])
def test_known_answers_and_shapes_that_stress_the_schedule(ea, ctx, name):
    ap, aj, want = _shape(name)
    out, st = check(ea, ctx, graph(ea, ap, aj), ap, aj, want)
    c = out.cpu().numpy()
    if name == "two_cliques_and_a_bridge":
        assert c.tolist() == [0] * 5 + [5] * 5 and want[2] == 40 / 42 - 0.5
    if name == "undo":
        assert want[3] == 2 and st.iterations == 3 and st.frontier_slots[:3] == [6, 0, 0]
    if name == "planted":
        assert (c == planted()[2] * 25).all() and want[1] == 20
    if "star" in name:
        assert (c == 0).all()
    if name == "isolated_and_self_loops":
        assert c.tolist() == [0, 1, 2, 3, 3, 5]
    if name == "no_entries":
        assert c.tolist() == list(range(9)) and st.iterations == 1 and st.edges_expanded == 0 and want[3] == 1
    if name == "triangle_among_isolated":
        assert want[1] == 201 and (c[[1, 100, 202]] == 1).all()
    if name == "triangles":
        assert (c.reshape(-1, 3) == c.reshape(-1, 3)[:, :1]).all() and (c[::3] == np.arange(0, 150000, 3)).all()
    if name == "shuffled_path":
        assert want[3] >= 5  # many levels: aggregation repeated on shrinking graphs


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    check(ea, ctx, g, ap, aj[: g.nnz])


_RMAT = {}


def _rmat(ea, ctx, scale=14):
    """(ap, aj, oracle answer) of the symmetric R-MAT multigraph as generated; computed once."""
    if scale not in _RMAT:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, _ = g.to_host()
        aj = aj[: g.nnz]
        _RMAT[scale] = (ap, aj, communities(ap, aj))
    return _RMAT[scale]


def test_rmat_multigraph_sorted_and_simple(ea, ctx):
    import torch
    ap, aj, want = _rmat(ea, ctx)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    out, st = check(ea, ctx, g, ap, aj, want)
    out = out.clone()
    # the same rows in another order: the same answer
    o2, n2, q2, l2, st2 = ea.louvain(ctx, g.sorted_rows(ctx))
    assert torch.equal(o2, out) and (n2, q2, l2) == want[1:4] and st2.iterations == st.iterations
    assert st2.frontier_slots == st.frontier_slots and st2.edges_expanded == st.edges_expanded
    # the simple graph counts every neighbour once: its own oracle run
    sap, saj = simple_csr(ap, aj)
    s = g.simple(ctx)
    assert s.nnz == len(saj)
    check(ea, ctx, s, sap, saj)


@pytest.mark.parametrize("hook,value", [("GRX_LOUVAIN_LDS_SLOTS", "64"), ("GRX_LOUVAIN_BIG_ROW", "8"),
                                        ("GRX_LOUVAIN_NARROW_EDGES", "0"), ("GRX_LOUVAIN_NARROW_EDGES", "1073741824")])
def test_with_the_thresholds_forced(ea, ctx, monkeypatch, hook, value):
    import torch
    ap, aj, want = _rmat(ea, ctx)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    base = ea.louvain(ctx, g)[0].clone()
    monkeypatch.setenv(hook, value)
    out, _ = check(ea, ctx, g, ap, aj, want)
    assert torch.equal(out, base)
    monkeypatch.delenv(hook)


def test_two_hooks_at_once_send_every_long_row_through_the_global_table(ea, ctx, monkeypatch):
    ap, aj, want = _rmat(ea, ctx)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    monkeypatch.setenv("GRX_LOUVAIN_LDS_SLOTS", "64")
    monkeypatch.setenv("GRX_LOUVAIN_BIG_ROW", "8")
    check(ea, ctx, g, ap, aj, want)
    monkeypatch.setenv("GRX_LOUVAIN_NARROW_EDGES", "0")
    check(ea, ctx, g, ap, aj, want)


@pytest.mark.parametrize("narrow", ["16384", "0"])
def test_a_weighted_big_row_on_a_coarse_level(ea, ctx, monkeypatch, narrow):
    ap, aj, want = _shape("hub_of_cliques")
    lap, laj, law = level_graph(ap, aj, 1)
    assert np.diff(lap).max() > 64 and law.max() > 1 and want[3] >= 2
    monkeypatch.setenv("GRX_LOUVAIN_BIG_ROW", "64")
    monkeypatch.setenv("GRX_LOUVAIN_NARROW_EDGES", narrow)
    check(ea, ctx, graph(ea, ap, aj), ap, aj, want)
    monkeypatch.setenv("GRX_LOUVAIN_LDS_SLOTS", "64")  # ... and through the global table
    check(ea, ctx, graph(ea, ap, aj), ap, aj, want)


def _coarsens(fine, coarse):
    return len(np.unique(np.stack([fine, coarse], 1), axis=0)) == len(np.unique(fine))


def test_dendrogram_cuts(ea, ctx):
    ap, aj, full = _rmat(ea, ctx)
    assert full[3] > 2
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    rows = []
    for phases in (1, 2):
        want = communities(ap, aj, max_phases=phases)
        assert want[3] == phases and want[4] == full[4][:len(want[4])]
        out, _ = check(ea, ctx, g, ap, aj, want, options=ea.Options(max_iterations=phases))
        rows.append(out.cpu().numpy())
    rows.append(full[0])
    assert _coarsens(rows[0], rows[1]) and _coarsens(rows[1], rows[2])


def test_repeat_calls_null_outputs_and_a_callers_tensor(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, want = _rmat(ea, ctx)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    a, count, q, levels, st = ea.louvain(ctx, g)
    a = a.clone()
    b, count2, q2, levels2, st2 = ea.louvain(ctx, g)
    assert torch.equal(a, b) and (count, q, levels, st.iterations, st.frontier_slots, st.edges_expanded) == \
        (count2, q2, levels2, st2.iterations, st2.frontier_slots, st2.edges_expanded)
    # d_community NULL: the call works on an array of its own
    n, qq, lv = C.c_int64(-7), C.c_double(-7.0), C.c_int32(-7)
    assert load_library().grx_louvain(ctx._h, g._h, None, C.byref(n), C.byref(qq), C.byref(lv), None, None) == 0
    assert (n.value, qq.value, lv.value) == want[1:4]
    lv = C.c_int32(-7)
    assert load_library().grx_louvain(ctx._h, g._h, None, None, None, C.byref(lv), None, None) == 0
    assert lv.value == want[3]
    # a caller's tensor is filled in place
    mine = torch.full((g.n_rows,), -5, dtype=torch.int32, device="cuda")
    out, count3, q3, _, _ = ea.louvain(ctx, g, mine)
    assert out is mine and count3 == want[1] and q3 == want[2] and (mine.cpu().numpy() == want[0]).all()


def test_stats_with_kernel_time(ea, ctx):
    ap, aj, want = _rmat(ea, ctx)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    _, _, _, _, st = ea.louvain(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    assert st.frontier_slots == want[4][:64] and st.iterations == len(want[4])  # moves, never microseconds


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, _ = _shape("two_cliques_and_a_bridge")
    g = graph(ea, ap, aj)
    lib = load_library()
    assert lib.grx_louvain(ctx._h, g._h, None, None, None, None, None, None) == -1
    assert lib.grx_louvain(None, g._h, None, None, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.louvain(ctx, graph(ea, ap, aj, n_cols=11))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.louvain(ctx, g, options=ea.Options(max_iterations=-1))
    assert e.value.code == -1
    with pytest.raises(TypeError):
        ea.louvain(ctx, g, torch.empty(10, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.louvain(ctx, g, torch.empty(9, dtype=torch.int32, device="cuda"))


def test_directed_input_is_unsupported(ea, ctx):
    with pytest.raises(ea.EngineError) as e:
        ea.louvain(ctx, ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False))
    assert e.value.code == -3
    ap, aj, _ = _shape("two_cliques_and_a_bridge")
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.louvain(ctx, g)
    assert e.value.code == -3


def test_the_empty_graph(ea, ctx):
    g = graph(ea, np.zeros(1, np.int32), np.zeros(0, np.int32))
    out, count, q, levels, st = ea.louvain(ctx, g)
    assert out.numel() == 0 and count == 0 and q == 0.0 and levels == 0 and st.iterations == 0


def test_rmat16_invariants(ea, ctx):
    """The checker is numpy on the host, not the code under test."""
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    a, count, q, levels, st = ea.louvain(ctx, g)
    _, lpa_count, lpa_q, lpa_st = ea.lpa(ctx, g)
    print(f"RMAT-16: communities {count} Q {q:.6f} levels {levels} sweeps {st.iterations} kept {st.frontier_slots} "
          f"launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f}; grx_lpa on the same handle: communities "
          f"{lpa_count} Q {lpa_q:.6f} elapsed_ms {lpa_st.elapsed_ms:.3f}")  # recorded, not asserted
    ap, aj, _ = g.to_host()
    ap = ap.astype(np.int64)
    aj = aj[: g.nnz].astype(np.int64)
    n = g.n_rows
    label = a.cpu().numpy().astype(np.int64)
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    assert count == int((label == np.arange(n)).sum()) and st.vertices_reached == n - count
    assert q == modularity_parts(ap, aj, label)[2] == ea.modularity(ctx, g, a)[0]
    # every phase ends in a 0 slot, and only there
    slots = st.frontier_slots
    if st.iterations <= 64:
        assert len(slots) == st.iterations and slots[-1] == 0 and slots.count(0) == levels
    else:
        assert len(slots) == 64 and slots.count(0) <= levels
    assert st.edges_expanded >= st.iterations and st.edges_traversed == g.nnz
    assert q > modularity_parts(ap, aj, np.arange(n))[2]
