"""grx_truss (k-truss decomposition) against the set-based oracle of tests/truss_oracle.py, exactly:
known answers, chesapeake, a multigraph as given, unsorted R-MAT multigraphs, shapes at which the
schedule can go wrong (one word taking 10 000 decrements and a triangle losing two edges in one
generation, many levels in a row, a long inward wave of small generations, no triangle at all),
the thresholds forced, invariants on RMAT-16 and argument errors.  Every graph: iterations == the
distinct values, edges_traversed == m, max_truss == values.max()."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tc_oracle import simple_edges
from truss_oracle import KNOWN, csr, entry_values, known_csr, truss_numbers

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


def check(ea, ctx, g, ap, aj, want=None, options=None):
    """ea.truss(g) equals the oracle on (ap, aj); the stats are the answer's."""
    want, largest, levels = want or truss_numbers(ap, aj)
    values, got, st = ea.truss(ctx, g, options=options)
    assert str(values.dtype) == "torch.int32" and values.numel() == g.nnz == len(want)
    v = values.cpu().numpy()
    assert (v == want).all()
    assert got == largest == (int(v.max()) if len(v) else 0)
    assert st.iterations == levels
    assert st.edges_traversed == len(simple_edges(ap, aj)[0])
    return v, st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, want = known_csr(name)
    v, st = check(ea, ctx, graph(ea, ap, aj), ap, aj)
    assert v.tolist() == want.tolist()
    assert st.iterations == len(set(want.tolist())) and st.edges_traversed == len(KNOWN[name][1])


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    v, st = check(ea, ctx, g, ap, aj)
    assert st.edges_traversed == 170 and set(v.tolist()) == {2, 3, 4, 5}


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def test_multigraph_as_given(ea, ctx):
    ap, aj = _random_multigraph()
    g = graph(ea, ap, aj)
    v, st = check(ea, ctx, g, ap, aj)
    assert st.edges_traversed == 345
    of = entry_values(ap, aj, v)
    for (a, b), seen in of.items():
        assert len(seen) == 1                      # every repeat carries the same value
        assert seen == ({0} if a == b else of[(b, a)])  # a loop 0, both directions equal
    assert any(a == b for a, b in of) and len(of) < len(aj)
    s = g.simple(ctx)
    sap, saj, _ = s.to_host()
    sv, largest, _ = ea.truss(ctx, s)
    simple = entry_values(sap, saj, sv.cpu().numpy())
    assert largest == int(v.max())
    assert simple == {e: t for e, t in of.items() if e[0] != e[1]}


_RMAT = {}


def _rmat(ea, ctx, scale):
    """(graph, ap, aj, the oracle's answer) of the R-MAT multigraph as generated, built once."""
    if scale not in _RMAT:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, _ = g.to_host()
        _RMAT[scale] = (g, ap, aj, truss_numbers(ap, aj))
    return _RMAT[scale]


@pytest.mark.parametrize("scale", [10, 12])
def test_rmat_as_generated(ea, ctx, scale):
    g, ap, aj, want = _rmat(ea, ctx, scale)
    v, _ = check(ea, ctx, g, ap, aj, want)
    src = np.repeat(np.arange(g.n_rows), np.diff(ap))
    assert (src == aj).any() and (v[src == aj] == 0).all() and (v[src != aj] >= 2).all()


def _book(pages=5000):
    edges = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    for p in range(5, 5 + pages):
        edges += [(0, p), (1, p)]
    return 5 + pages, edges


def _clique_ladder():
    edges, first, last = [], 0, None
    for size in range(3, 41):
        edges += [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]
        if last is not None:
            edges.append((last, first))
        last = first + size - 1
        first += size
    return first, edges


def _triangular_grid(side=200):
    at = lambda r, c: r * side + c  # noqa: E731
    edges = [(at(r, c), at(r, c + 1)) for r in range(side) for c in range(side - 1)]
    edges += [(at(r, c), at(r + 1, c)) for r in range(side - 1) for c in range(side)]
    edges += [(at(r, c), at(r + 1, c + 1)) for r in range(side - 1) for c in range(side - 1)]
    return side * side, edges


def _path():
    n = 20001
    return n, [(i, i + 1) for i in range(n - 1)]


def _isolated_and_a_triangle():
    return 70003, [(70000, 70001), (70001, 70002), (70002, 70000)]


SHAPES = {"book": _book, "clique_ladder": _clique_ladder, "triangular_grid": _triangular_grid, "path": _path,
          "isolated_and_a_triangle": _isolated_and_a_triangle}


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(ap, aj, the oracle's answer) of a shape, built once."""
    n, edges = SHAPES[name]()
    ap, aj = csr(n, np.asarray(edges, np.int64))
    return ap, aj, truss_numbers(ap, aj)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_at_which_the_schedule_can_go_wrong(ea, ctx, name):
    ap, aj, want = _shape(name)
    v, st = check(ea, ctx, graph(ea, ap, aj), ap, aj, want)
    src = np.repeat(np.arange(len(ap) - 1), np.diff(ap))
    if name == "book":
        in_k5 = (src < 5) & (aj < 5)
        assert (v[in_k5] == 5).all() and (v[~in_k5] == 3).all() and st.iterations == 2
    if name == "clique_ladder":
        size_of = np.repeat(np.arange(3, 41), np.arange(3, 41))  # the clique a vertex lies in
        bridge = size_of[src] != size_of[aj]
        assert (v[bridge] == 2).all() and (v[~bridge] == size_of[src][~bridge]).all()
        assert st.iterations == 39
    if name == "triangular_grid":
        assert (v == 3).all() and st.iterations == 1
    if name == "path":
        assert (v == 2).all() and st.iterations == 1
    if name == "isolated_and_a_triangle":
        assert v.tolist() == [3] * 6 and st.edges_traversed == 3


@pytest.mark.parametrize("hook,value", [("GRX_TRUSS_NARROW_EDGES", "0"), ("GRX_TRUSS_NARROW_EDGES", "1000000000"),
                                        ("GRX_TRUSS_LDS_IDS", "64"), ("GRX_TRUSS_LDS_IDS", "8")])
@pytest.mark.parametrize("which", ["rmat12", "book"])
def test_with_the_thresholds_forced(ea, ctx, monkeypatch, which, hook, value):
    if which == "rmat12":
        g, ap, aj, want = _rmat(ea, ctx, 12)
    else:
        ap, aj, want = _shape("book")
        g = graph(ea, ap, aj)
    base, largest, st = ea.truss(ctx, g)
    base = base.cpu().numpy()
    monkeypatch.setenv(hook, value)
    v, st2 = check(ea, ctx, g, ap, aj, want)
    assert (v == base).all() and st2.edges_expanded == st.edges_expanded
    if hook == "GRX_TRUSS_NARROW_EDGES":
        # the schedule did change: all generations in launches of their own, or none
        assert (st2.advance_launches > st.advance_launches) == (value == "0")


def test_rmat16_invariants(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    a, largest, st = ea.truss(ctx, g, options=ea.Options(collect_kernel_time=True))
    a = a.clone()
    b, largest2, st2 = ea.truss(ctx, g)
    assert torch.equal(a, b) and largest == largest2 == int(a.max()) > 2
    assert st.iterations == st2.iterations == a[a > 0].unique().numel()
    assert st.edges_expanded == st2.edges_expanded
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    assert len(st.frontier_slots) == 3 and all(t > 0 for t in st.frontier_slots)
    assert sum(st.frontier_slots) <= st.advance_kernel_ms * 1000 + 3
    ap, aj, _ = g.to_host()
    n = g.n_rows
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    key = src * n + aj
    v = a.cpu().numpy()
    assert st.edges_traversed == len(simple_edges(ap, aj)[0])
    assert (v[src == aj] == 0).all()
    # the simple graph, edge by edge: its sorted rows make its keys ascending
    s = g.simple(ctx)
    sap, saj, _ = s.to_host()
    sv, largest3, st3 = ea.truss(ctx, s)
    sv = sv.cpu().numpy()
    skey = np.repeat(np.arange(n, dtype=np.int64), np.diff(sap)) * n + saj
    assert largest3 == largest and st3.iterations == st.iterations and st3.edges_traversed == st.edges_traversed
    assert 2 * st.edges_traversed == len(saj)
    at = np.searchsorted(skey, key[src != aj])
    assert (skey[at] == key[src != aj]).all() and (sv[at] == v[src != aj]).all()
    # both directions agree
    back = np.searchsorted(skey, saj.astype(np.int64) * n + np.repeat(np.arange(n, dtype=np.int64), np.diff(sap)))
    assert (sv[back] == sv).all()
    g.hot_first(ctx, True)
    c, largest4, _ = ea.truss(ctx, g)
    assert torch.equal(c, a) and largest4 == largest


def test_values_tensor_is_validated(ea, ctx):
    import torch
    ap, aj, want = known_csr("complete5")
    g = graph(ea, ap, aj)
    out = torch.full((g.nnz,), -1, dtype=torch.int32, device="cuda")
    v, largest, _ = ea.truss(ctx, g, values=out)
    assert v is out and out.cpu().numpy().tolist() == want.tolist() and largest == 5
    with pytest.raises(TypeError):
        ea.truss(ctx, g, values=torch.zeros(g.nnz, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ea.truss(ctx, g, values=torch.zeros(g.n_rows, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ea.truss(ctx, g, values=torch.zeros(g.nnz, dtype=torch.int32))


def test_argument_errors(ea, ctx):
    from essentials_amd.api import load_library
    ap, aj, _ = known_csr("complete5")
    g = graph(ea, ap, aj)
    assert load_library().grx_truss(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.truss(ctx, graph(ea, ap, aj, n_cols=6))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.truss(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    d = C.c_int32(-7)
    assert load_library().grx_truss(ctx._h, g._h, None, C.byref(d), None, None) == 0
    assert d.value == 5


def test_directed_input_is_unsupported(ea, ctx):
    rng = np.random.default_rng(5)
    ap, aj = csr(50, rng.integers(0, 50, size=(200, 2)), symmetric=False)
    with pytest.raises(ea.EngineError) as e:
        ea.truss(ctx, graph(ea, ap, aj))
    assert e.value.code == -3 and "directed" in str(e.value)
    ap, aj, _ = known_csr("complete12")
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.truss(ctx, g)
    assert e.value.code == -3
