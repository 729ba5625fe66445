"""grx_tc (triangle counting) against the numpy oracle of tests/tc_oracle.py, per vertex: the
reference unit test's known answers, small edge cases, chesapeake, unsorted R-MAT multigraphs,
the path for rows that do not fit LDS, the unchanged tc.hxx when built, argument errors and
invariants on RMAT-22."""
import ctypes as C
from math import comb
import os

import numpy as np
import pytest

from tc_oracle import KNOWN, KNOWN_COUNTS, KNOWN_T, csr, mtx_csr, triangles

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


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, ap, aj):
    want, t = triangles(ap, aj)
    counts, got_t, st = ea.tc(ctx, g)
    assert str(counts.dtype) == "torch.int64"
    assert (counts.cpu().numpy() == want).all()
    assert got_t == t and st.iterations == 1
    assert ea.tc(ctx, g, per_vertex=False)[1] == t
    return counts, t, st


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ea, ctx, name):
    ap, aj = (np.array(x, np.int32) for x in KNOWN[name])
    counts, t, st = ea.tc(ctx, graph(ea, ap, aj))
    assert counts.cpu().numpy().tolist() == KNOWN_COUNTS and t == KNOWN_T
    assert st.edges_traversed == 5


def _k4_repeated_shuffled():
    rng = np.random.default_rng(2)
    e = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    ap, aj = csr(4, e * 3)
    for u in range(4):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return 4, ap, aj


SMALL = {
    "empty": lambda: (1, *csr(1, np.zeros((0, 2)))),
    "isolated": lambda: (9, *csr(9, np.zeros((0, 2)))),
    "triangle": lambda: (3, *csr(3, [(0, 1), (1, 2), (2, 0)])),
    "k4": lambda: (4, *csr(4, [(a, b) for a in range(4) for b in range(a + 1, 4)])),
    "k40": lambda: (40, *csr(40, [(a, b) for a in range(40) for b in range(a + 1, 40)])),
    "star": lambda: (30, *csr(30, [(0, i) for i in range(1, 30)])),
    "path": lambda: (30, *csr(30, [(i, i + 1) for i in range(29)])),
    "self_loops_only": lambda: (6, *csr(6, [(i, i) for i in range(6)], symmetric=False)),
    "k4_repeated_shuffled": _k4_repeated_shuffled,
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs(ea, ctx, name):
    n, ap, aj = SMALL[name]()
    counts, t, _ = check(ea, ctx, graph(ea, ap, aj), ap, aj)
    if name == "k40":
        assert (counts.cpu().numpy() == comb(39, 2)).all() and t == comb(40, 3)
    if name == "k4_repeated_shuffled":
        assert counts.cpu().numpy().tolist() == [3, 3, 3, 3] and t == 4


def test_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(os.path.join(GOLDEN_DIR, "chesapeake.mtx"))
    ap, aj, _ = g.to_host()
    _, t, _ = check(ea, ctx, g, ap, aj)
    assert t == triangles(*mtx_csr(os.path.join(GOLDEN_DIR, "chesapeake.mtx")))[1]


@pytest.mark.parametrize("scale", [16, 18])
def test_rmat_unsorted_multigraph(ea, ctx, scale):
    import torch
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    ap, aj, ax = g.to_host()
    want, t = triangles(ap, aj)
    counts, got_t, st = ea.tc(ctx, g)
    assert (counts.cpu().numpy() == want).all() and got_t == t
    # the same arrays as a non-owning view (symmetry unknown: verified on the call)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ap, aj[: g.nnz], ax[: g.nnz])]
    v = ea.Graph.from_device_csr(*dev)
    c2, t2, st2 = ea.tc(ctx, v)
    assert torch.equal(c2, counts) and t2 == t
    assert st2.edges_traversed == st.edges_traversed and st2.edges_expanded == st.edges_expanded


def test_rows_that_miss_lds(ea, ctx, monkeypatch):
    import torch
    g = ea.Graph.rmat(ctx, 16, 16, 1, 7)
    base, t, _ = ea.tc(ctx, g)
    base = base.clone()
    for cap in ("100", "30", "1"):  # the longest oriented rows of RMAT-16 are longer than 100
        monkeypatch.setenv("GRX_TC_LDS_IDS", cap)
        counts, t2, _ = ea.tc(ctx, g)
        assert torch.equal(counts, base) and t2 == t, cap


def _dedup_sorted(g, torch):
    """The graph's CSR with repeats dropped and self loops kept, rows sorted: unique(row * n + col)."""
    ap, aj, _ = g.to_host()
    n = g.n_rows
    ap_d = torch.from_numpy(ap.astype(np.int64)).cuda()
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), ap_d[1:] - ap_d[:-1])
    key = torch.unique(row * n + torch.from_numpy(aj[: g.nnz].astype(np.int64)).cuda())
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(key // n, minlength=n), 0)
    return off.int(), (key % n).int()


def test_unchanged_tc_hxx_on_sorted_rmat20(ea, ctx):
    import torch
    from oracle.oracle import RefClients
    if not RefClients.available() or not hasattr(C.CDLL(RefClients._path()), "refc_tc"):
        pytest.skip("the reference clients library with refc_tc was not built")
    g = ea.Graph.rmat(ctx, 20, 16, 1, 7)
    off, col = _dedup_sorted(g, torch)
    # rows without repeats: the largest simple degree is below 2^16, so C(d, 2) < 2^31
    assert int((off[1:] - off[:-1]).max()) < 65536
    val = torch.ones(col.numel(), dtype=torch.float32, device="cuda")
    ref_counts = torch.zeros(g.n_rows, dtype=torch.int32, device="cuda")
    total = RefClients().tc(off, col, val, ref_counts)
    torch.cuda.synchronize()
    counts, t, _ = ea.tc(ctx, ea.Graph.from_device_csr(off, col, val))
    assert torch.equal(ref_counts.long(), counts)
    assert total == 3 * t
    counts2, t2, _ = ea.tc(ctx, g)  # the unsorted multigraph it came from: the same answer
    assert torch.equal(counts2, counts) and t2 == t


def test_directed_input_is_unsupported(ea, ctx):
    rng = np.random.default_rng(5)
    ap, aj = csr(50, rng.integers(0, 50, size=(200, 2)), symmetric=False)
    with pytest.raises(ea.EngineError) as e:
        ea.tc(ctx, graph(ea, ap, aj))
    assert e.value.code == -3
    ap, aj = csr(40, [(a, b) for a in range(40) for b in range(a + 1, 40)])
    g = graph(ea, ap, aj)
    g.build_in_edges(ctx)
    with pytest.raises(ea.EngineError) as e:
        ea.tc(ctx, g)
    assert e.value.code == -3


def test_argument_errors(ea, ctx):
    from essentials_amd.api import load_library
    ap, aj = csr(4, [(a, b) for a in range(4) for b in range(a + 1, 4)])
    g = graph(ea, ap, aj)
    assert load_library().grx_tc(ctx._h, g._h, None, None, None, None) == -1
    with pytest.raises(ea.EngineError) as e:
        ea.tc(ctx, graph(ea, ap, aj, n_cols=5))
    assert e.value.code == -1
    counts, t, _ = ea.tc(ctx, g, per_vertex=False)
    assert counts is None and t == 4


def test_rmat22_invariants(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
    a, t, st = ea.tc(ctx, g, options=ea.Options(collect_kernel_time=True))
    a = a.clone()
    b, t2, _ = ea.tc(ctx, g)
    assert torch.equal(a, b) and t == t2 and t > 0
    assert int(a.sum()) == 3 * t
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms
    off, col = _dedup_sorted(g, torch)
    n = g.n_rows
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), (off[1:] - off[:-1]).long())
    d = torch.bincount(row[row != col.long()], minlength=n)  # simple degree
    assert st.edges_traversed * 2 == int(d.sum())
    assert bool((a <= d * (d - 1) // 2).all())
    assert bool((a[d < 2] == 0).all())
    g.hot_first(ctx, True)
    c, t3, _ = ea.tc(ctx, g)
    assert torch.equal(c, a) and t3 == t
