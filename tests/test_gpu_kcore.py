"""grx_kcore (k-core decomposition) and grx_graph_simple against the numpy oracle of
tests/kcore_oracle.py, exactly: known answers, chesapeake (and the reference's own harness when
built), unsorted R-MAT multigraphs and their simple graphs, shapes that stress the schedule (long
chains of tiny rounds, many thin levels, one huge row, queues that outgrow the one-workgroup
kernel), argument errors and invariants on RMAT-22.  Every graph: edges_expanded == nnz."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kcore_oracle import KNOWN, core_numbers, csr, known_csr, simple_csr, write_mtx

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
REF_KCORE = os.path.join(ROOT, "oracle", "_ref", "ref_kcore")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, ap, aj):
    """ea.kcore(g) equals the oracle on (ap, aj); the stats are the answer's, the work is nnz."""
    want, degeneracy, levels = core_numbers(ap, aj)
    cores, got, st = ea.kcore(ctx, g)
    assert str(cores.dtype) == "torch.int32"
    assert (cores.cpu().numpy() == want).all()
    assert got == degeneracy and st.iterations == levels
    assert st.edges_expanded == g.nnz == st.edges_traversed
    assert st.vertices_reached == int((np.diff(np.asarray(ap, np.int64)) > 0).sum())
    return cores, st


def ref_values(path):
    """The first 40 core numbers ref_kcore prints for a Matrix Market file, GPU and CPU."""
    r = subprocess.run([REF_KCORE, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Number of errors : 0" in r.stdout, r.stdout[-1500:]
    out = []
    for head in ("GPU k-core values[:", "CPU k-core values[:"):
        line = [l for l in r.stdout.splitlines() if l.startswith(head)][0]
        out.append([int(x) for x in line.split("=")[1].split()])
    return out


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj, want = known_csr(name)
    cores, st = check(ea, ctx, graph(ea, ap, aj), ap, aj)
    assert cores.cpu().numpy().tolist() == want.tolist()
    assert st.iterations == len(set(want[want > 0].tolist()))


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    cores, _ = check(ea, ctx, g, ap, aj)
    if not os.path.exists(REF_KCORE):
        pytest.skip("oracle/_ref/ref_kcore not built (reference tree was not mounted)")
    gpu, cpu = ref_values(CHESAPEAKE)
    assert gpu == cpu == cores.cpu().numpy().tolist()[:40] and len(gpu) == 39


@pytest.mark.parametrize("scale", [16, 18, 20])
def test_rmat_multigraph_as_generated(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    ap, aj, ax = g.to_host()
    cores, st = check(ea, ctx, g, ap, aj)
    if scale == 16:  # the same arrays as a non-owning view (symmetry unknown: verified on the call)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ap, aj, ax)]
        c2, d2, st2 = ea.kcore(ctx, ea.Graph.from_device_csr(*dev))
        assert torch.equal(c2, cores) and d2 == int(cores.max())
        assert st2.iterations == st.iterations and st2.edges_expanded == g.nnz


@pytest.mark.parametrize("scale", [16, 18])
def test_simple_graph(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    ap, aj, ax = g.to_host()
    sap, saj, sax = simple_csr(ap, aj, ax)
    s = g.simple(ctx)
    gap, gaj, gax = s.to_host()
    assert s.nnz == len(saj) and (gap == sap).all() and (gaj == saj).all() and (gax == sax).all()
    check(ea, ctx, s, sap, saj)
    a, t, _ = ea.tc(ctx, g)
    b, t2, _ = ea.tc(ctx, s)
    assert torch.equal(a, b) and t == t2


def test_simple_rmat16_through_the_reference_harness(ea, ctx, tmp_path):
    if not os.path.exists(REF_KCORE):
        pytest.skip("oracle/_ref/ref_kcore not built (reference tree was not mounted)")
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    ap, aj, _ = g.to_host()
    sap, saj = simple_csr(ap, aj)
    path = str(tmp_path / "rmat16_simple.mtx")
    write_mtx(path, sap, saj)
    gpu, cpu = ref_values(path)
    cores, _, _ = ea.kcore(ctx, ea.Graph.from_mtx(path))
    assert gpu == cpu == cores.cpu().numpy().tolist()[:40]
    assert (cores.cpu().numpy() == core_numbers(sap, saj)[0]).all()


def _path():
    n = 20001
    return n, [(i, i + 1) for i in range(n - 1)]


def _clique_ladder():
    edges, first, last = [], 0, None
    for size in range(3, 61):
        edges += [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]
        if last is not None:
            edges.append((last, first))
        last = first + size - 1
        first += size
    return first, edges


def _star_with_clique():
    leaves = 300000
    edges = [(0, i) for i in range(1, 40)] + [(a, b) for a in range(1, 40) for b in range(a + 1, 40)]
    edges += [(0, 40 + i) for i in range(leaves)]
    return 40 + leaves, edges


def _grid():
    side = 300
    at = lambda r, c: r * side + c  # noqa: E731
    edges = [(at(r, c), at(r, c + 1)) for r in range(side) for c in range(side - 1)]
    edges += [(at(r, c), at(r + 1, c)) for r in range(side - 1) for c in range(side)]
    return side * side, edges


def _isolated_and_a_triangle():
    return 70003, [(70000, 70001), (70001, 70002), (70002, 70000)]


SHAPES = {"path": _path, "clique_ladder": _clique_ladder, "star_with_clique": _star_with_clique, "grid": _grid,
          "isolated_and_a_triangle": _isolated_and_a_triangle}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_that_stress_the_schedule(ea, ctx, name):
    n, edges = SHAPES[name]()
    ap, aj = csr(n, np.asarray(edges, np.int64))
    cores, st = check(ea, ctx, graph(ea, ap, aj), ap, aj)
    c = cores.cpu().numpy()
    if name == "path":
        assert (c == 1).all()
    if name == "grid":
        assert (c == 2).all()
    if name == "clique_ladder":
        assert sorted(set(c.tolist())) == list(range(2, 60)) and st.iterations == 58
    if name == "star_with_clique":
        assert c[0] == 39 and (c[1:40] == 39).all() and (c[40:] == 1).all()
    if name == "isolated_and_a_triangle":
        assert (c[:70000] == 0).all() and (c[70000:] == 2).all() and st.vertices_reached == 3


@pytest.mark.parametrize("hook,value", [("GRX_KCORE_NARROW_EDGES", "1"), ("GRX_KCORE_NARROW_EDGES", "1000000000"),
                                        ("GRX_KCORE_BIG_ROW", "1"), ("GRX_KCORE_BIG_ROW", "1000000000")])
def test_rmat16_with_the_thresholds_forced(ea, ctx, monkeypatch, hook, value):
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    base, d, st = ea.kcore(ctx, g)
    base = base.clone()
    monkeypatch.setenv(hook, value)
    cores, d2, st2 = ea.kcore(ctx, g)
    assert torch.equal(cores, base) and d2 == d
    assert st2.iterations == st.iterations and st2.edges_expanded == g.nnz == st.edges_expanded


def test_argument_errors(ea, ctx):
    from essentials_amd.api import load_library
    ap, aj, _ = known_csr("complete5")
    g = graph(ea, ap, aj)
    assert load_library().grx_kcore(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.kcore(ctx, graph(ea, ap, aj, n_cols=6))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.kcore(ctx, g, options=ea.Options(max_iterations=3))
    assert e.value.code == -1
    d = C.c_int32(-7)
    assert load_library().grx_kcore(ctx._h, g._h, None, C.byref(d), None, None) == 0
    assert d.value == 4


def test_directed_input_is_unsupported(ea, ctx):
    rng = np.random.default_rng(5)
    ap, aj = csr(50, rng.integers(0, 50, size=(200, 2)), symmetric=False)
    with pytest.raises(ea.EngineError) as e:
        ea.kcore(ctx, graph(ea, ap, aj))
    assert e.value.code == -3
    ap, aj, _ = known_csr("complete12")
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.kcore(ctx, g)
    assert e.value.code == -3


def test_rmat22_invariants(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
    a, d, st = ea.kcore(ctx, g, options=ea.Options(collect_kernel_time=True))
    a = a.clone()
    b, d2, _ = ea.kcore(ctx, g)
    assert torch.equal(a, b) and d == d2
    assert d == int(a.max()) > 0
    assert st.iterations == a[a > 0].unique().numel()
    assert st.edges_expanded == g.nnz
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    ap, aj, _ = g.to_host()
    off = torch.from_numpy(ap.astype(np.int64)).cuda()
    length = off[1:] - off[:-1]
    assert torch.equal(a == 0, length == 0)
    # membership certificate: v has at least cores[v] entries that name a vertex of its core
    row = torch.repeat_interleave(torch.arange(g.n_rows, device="cuda"), length)
    col = torch.from_numpy(aj.astype(np.int64)).cuda()
    support = torch.bincount(row[a[col] >= a[row]], minlength=g.n_rows)
    assert bool((support >= a).all())
    del row, col, support
    assert (a.cpu().numpy() == core_numbers(ap, aj)[0]).all()
    g.hot_first(ctx, True)
    c, d3, _ = ea.kcore(ctx, g)
    assert torch.equal(c, a) and d3 == d
