"""grx_color (greedy colouring, largest degree first) against the numpy oracle of
tests/color_oracle.py, exactly: known answers, chesapeake, unsorted R-MAT multigraphs with their
sorted and simple copies, shapes that stress the schedule (colours beyond a 64-bit mask, one
contended counter and a big row, thousands of tiny generations, queues that outgrow the
one-workgroup kernel), the test hooks, the stats, argument errors and invariants on RMAT-20.
Every graph: iterations == depth of the priority DAG and edges_expanded == 2 * nnz."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from color_oracle import KNOWN, colouring, csr, known_csr, simple_csr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
HOOKS = ("GRX_COLOR_NARROW_EDGES", "GRX_COLOR_BIG_ROW", "GRX_COLOR_MEX_WINDOW")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, ap, aj, want=None):
    """ea.color(g) equals the oracle on (ap, aj); the stats are the answer's."""
    want = want or colouring(ap, aj)
    colors, count, st = ea.color(ctx, g)
    assert str(colors.dtype) == "torch.int32" and colors.numel() == g.n_rows
    host = colors.cpu().numpy()
    print(f"V {g.n_rows} nnz {g.nnz} colours {count} (oracle {want[1]}) iterations {st.iterations} (oracle {want[2]}) "
          f"edges_expanded {st.edges_expanded} launches {st.advance_launches} elapsed_ms {st.elapsed_ms:.3f} "
          f"mismatches {int((host != want[0]).sum())}")
    assert (host == want[0]).all()
    assert count == want[1] and st.iterations == want[2]
    assert st.edges_expanded == 2 * g.nnz and st.edges_traversed == g.nnz
    assert st.vertices_reached == int((np.diff(np.asarray(ap, np.int64)) > 0).sum())
    assert st.advance_kernel_ms == 0
    return colors, st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, want = known_csr(name)
    colors, _ = check(ea, ctx, graph(ea, ap, aj), ap, aj)
    assert colors.cpu().numpy().tolist() == want.tolist()


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    check(ea, ctx, g, ap, aj)


_RMAT = {}


def _rmat(ea, ctx, scale):
    """(ap, aj, oracle answer) of the symmetric R-MAT multigraph as generated; computed once."""
    if scale not in _RMAT:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, _ = g.to_host()
        aj = aj[: g.nnz]
        _RMAT[scale] = (ap, aj, colouring(ap, aj))
    return _RMAT[scale]


@pytest.mark.parametrize("scale", [12, 14, 16])
def test_rmat_multigraph_sorted_and_simple(ea, ctx, scale):
    import torch
    ap, aj, want = _rmat(ea, ctx, scale)
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    colors, st = check(ea, ctx, g, ap, aj, want)
    colors = colors.clone()
    # the same degrees in another row order: the same answer
    c2, n2, st2 = ea.color(ctx, g.sorted_rows(ctx))
    assert torch.equal(c2, colors) and n2 == want[1] and st2.iterations == st.iterations
    assert st2.edges_expanded == 2 * g.nnz
    # the simple graph has other degrees: its own oracle run
    sap, saj = simple_csr(ap, aj)
    s = g.simple(ctx)
    assert s.nnz == len(saj)
    check(ea, ctx, s, sap, saj)


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def _k300_pendants():
    return 1300, _clique(300) + [(i % 300, 300 + i) for i in range(1000)]


def _star(hub_last):
    leaves = 300000
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


def _isolated_and_a_triangle():
    return 70003, [(70000, 70001), (70001, 70002), (70002, 70000)]


def _repeats_and_a_self_loop():
    return 3, [(0, 1)] * 5000 + [(0, 0), (1, 2)]


SHAPES = {"k70": lambda: (70, _clique(70)), "k300": lambda: (300, _clique(300)), "k300_pendants": _k300_pendants,
          "star_hub_first": lambda: _star(False), "star_hub_last": lambda: _star(True),
          "shuffled_path": _shuffled_path, "grid": _grid, "triangles": _triangles,
          "isolated_and_a_triangle": _isolated_and_a_triangle, "repeats_and_a_self_loop": _repeats_and_a_self_loop}


@functools.lru_cache(maxsize=None)
def _shape(name):
    n, edges = SHAPES[name]()
    ap, aj = csr(n, np.asarray(edges, np.int64))
    return ap, aj, colouring(ap, aj)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_that_stress_the_schedule(ea, ctx, name):
    ap, aj, want = _shape(name)
    colors, st = check(ea, ctx, graph(ea, ap, aj), ap, aj, want)
    c = colors.cpu().numpy()
    if name in ("k70", "k300"):
        assert sorted(c.tolist()) == list(range(len(c))) and st.iterations == len(c)
    if name == "k300_pendants":
        assert sorted(c[:300].tolist()) == list(range(300)) and (c[300:] <= 1).all()
    if name == "star_hub_first":
        assert c[0] == 0 and (c[1:] == 1).all() and st.iterations == 2
    if name == "star_hub_last":
        assert c[-1] == 0 and (c[:-1] == 1).all() and st.iterations == 2
    if name in ("shuffled_path", "grid"):
        assert c.max() <= 2 + (name == "grid") * 2
    if name == "triangles":
        assert (np.sort(c.reshape(-1, 3), 1) == [0, 1, 2]).all() and st.iterations == 3
    if name == "isolated_and_a_triangle":
        assert (c[:70000] == 0).all() and sorted(c[70000:].tolist()) == [0, 1, 2] and st.vertices_reached == 3
    if name == "repeats_and_a_self_loop":
        assert c.tolist() == [0, 1, 0]


def _hooked_graph(ea, ctx, name):
    if name == "rmat14":
        return ea.Graph.rmat(ctx, 14, 16, 1, 7), _rmat(ea, ctx, 14)[2]
    ap, aj, want = _shape(name)
    return graph(ea, ap, aj), want


@pytest.mark.parametrize("window", ["64", None])
@pytest.mark.parametrize("big_row", ["1", "1000000000"])
@pytest.mark.parametrize("narrow", ["0", None])
@pytest.mark.parametrize("name", ["rmat14", "k300", "star_hub_first", "star_hub_last"])
def test_with_the_thresholds_forced(ea, ctx, monkeypatch, name, narrow, big_row, window):
    import torch
    for hook in HOOKS:
        monkeypatch.delenv(hook, raising=False)
    g, want = _hooked_graph(ea, ctx, name)
    base, count, st = ea.color(ctx, g)
    base = base.clone()
    assert (base.cpu().numpy() == want[0]).all()
    for hook, value in zip(HOOKS, (narrow, big_row, window)):
        if value is not None:
            monkeypatch.setenv(hook, value)
    colors, count2, st2 = ea.color(ctx, g)
    assert torch.equal(colors, base) and count2 == count == want[1]
    assert st2.iterations == st.iterations == want[2]
    assert st2.edges_expanded == 2 * g.nnz == st.edges_expanded
    if narrow == "0" and big_row == "1000000000":  # a wide launch per generation, the batch's init and hand-offs
        assert st2.advance_launches == 4 + 2 * want[2]


def test_stats(ea, ctx):
    ap, aj, want = _rmat(ea, ctx, 14)
    g = ea.Graph.rmat(ctx, 14, 16, 1, 7)
    _, _, st = ea.color(ctx, g, options=ea.Options(collect_kernel_time=True))
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    assert st.vertices_reached == int((np.diff(ap.astype(np.int64)) > 0).sum())
    _, _, st = ea.color(ctx, g)
    assert st.advance_kernel_ms == 0 and st.elapsed_ms > 0 and st.advance_launches >= 4


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    ap, aj, want = known_csr("triangle_with_pendants")
    g = graph(ea, ap, aj)
    assert load_library().grx_color(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.color(ctx, graph(ea, ap, aj, n_cols=10))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.color(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    with pytest.raises(TypeError):
        ea.color(ctx, g, torch.empty(9, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.color(ctx, g, torch.empty(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ea.color(ctx, g, torch.empty(18, dtype=torch.int32, device="cuda")[::2])
    with pytest.raises(ValueError):
        ea.color(ctx, g, torch.empty(9, dtype=torch.int32))
    # the count alone: the call works on an array of its own
    n = C.c_int32(-7)
    assert load_library().grx_color(ctx._h, g._h, None, C.byref(n), None, None) == 0
    assert n.value == 3
    # a caller's tensor is filled in place
    mine = torch.full((9,), -5, dtype=torch.int32, device="cuda")
    out, count, _ = ea.color(ctx, g, mine)
    assert out is mine and count == 3 and mine.cpu().tolist() == want.tolist()


def test_directed_input_is_unsupported(ea, ctx):
    with pytest.raises(ea.EngineError) as e:
        ea.color(ctx, ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False))
    assert e.value.code == -3
    ap, aj, _ = known_csr("complete12")
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.color(ctx, g)
    assert e.value.code == -3


def test_rmat20_invariants(ea, ctx):
    """The checker is torch, not the code under test."""
    import torch
    g = ea.Graph.rmat(ctx, 20, 16, 1, 7)
    a, count, st = ea.color(ctx, g)
    a = a.clone()
    b, count2, st2 = ea.color(ctx, g)
    assert torch.equal(a, b) and count == count2 and st.iterations == st2.iterations
    assert st.edges_expanded == 2 * g.nnz
    print(f"RMAT-20: colours {count} iterations {st.iterations} launches {st.advance_launches} "
          f"elapsed_ms {st.elapsed_ms:.3f}")
    ap, aj, _ = g.to_host()
    off = torch.from_numpy(ap.astype(np.int64)).cuda()
    length = off[1:] - off[:-1]
    row = torch.repeat_interleave(torch.arange(g.n_rows, device="cuda"), length)
    col = torch.from_numpy(aj[: g.nnz].astype(np.int64)).cuda()
    la = a.long()
    off_diagonal = row != col
    assert bool((la[row] != la[col])[off_diagonal].all())
    assert bool((la >= 0).all()) and bool((la <= length).all())
    assert count == int(la.max()) + 1
    # colour 0 is a maximal independent set: every other vertex has a neighbour of colour 0
    sees_zero = torch.zeros(g.n_rows, dtype=torch.bool, device="cuda")
    sees_zero[row[off_diagonal & (la[col] == 0)]] = True
    assert bool((sees_zero | (la == 0)).all())
