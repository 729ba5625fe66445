"""Pulled wide levels of the default BFS client (bfs_enactor_t::expand): on a
graph KNOWN to be symmetric a label-scan level that passes Beamer's test lets every unlabelled vertex
look for one frontier neighbour (pull_range_kernel) instead of expanding the frontier.

Every case compares depths exactly with oracle.bfs_heap on the graph's own arrays, and every pulled
run with a GRX_BFS_PULL=0 run of the same call: a pulled level finds the same set, so the depths and
(iterations, vertices_reached, edges_traversed, edges_expanded, frontier_slots) are equal.  The
thresholds are forced down at context creation so that every level with a work hint is a label-scan
level, and do_alpha=1e9 makes each of them pull.  Level 0 (the source alone) carries no work hint and
always pushes, so a search that ends after it has no pulled level.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

INF_I = 2**31 - 1
FORCED = {"GRX_SETTLED_MIN_WORK": "1", "GRX_FUSED_MIN_SLOTS": "64", "GRX_LABEL_SCAN_MIN_WORK": "1"}
PER_CALL = ("GRX_BFS_PULL", "GRX_BFS_BYTE_LABELS", "GRX_BFS_MARK")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def gpu(oracle, monkeypatch):
    import torch
    import essentials_amd as ea
    assert torch.cuda.is_available()
    for name in PER_CALL + tuple(FORCED) + ("GRX_HOT_FIRST",):
        monkeypatch.delenv(name, raising=False)
    return ea


def forced_context(ea, monkeypatch):
    """The thresholds are read when a context is made."""
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    ctx = ea.Context(0)
    for k in FORCED:
        monkeypatch.delenv(k)
    return ctx


def key(st):
    return (st.iterations, st.vertices_reached, st.edges_traversed, st.edges_expanded, tuple(st.frontier_slots))


def run(ea, ctx, g, s, monkeypatch, options=None, byte_labels=None):
    """(depths, stats) of the call as it stands and of the same call with GRX_BFS_PULL=0."""
    out = []
    for pull in (None, "0"):   # unset: the default, which pulls
        if pull is None:
            monkeypatch.delenv("GRX_BFS_PULL", raising=False)
        else:
            monkeypatch.setenv("GRX_BFS_PULL", pull)
        if byte_labels is None:
            monkeypatch.delenv("GRX_BFS_BYTE_LABELS", raising=False)
        else:
            monkeypatch.setenv("GRX_BFS_BYTE_LABELS", str(int(byte_labels)))
        d, st = ea.bfs(ctx, g, s, options=options)
        out.append((d.cpu().numpy(), st))
    for name in PER_CALL:
        monkeypatch.delenv(name, raising=False)
    return out


def check_pulled(tag, ea, ctx, g, s, want, monkeypatch, must_pull=True, **how):
    (d1, st1), (d0, st0) = run(ea, ctx, g, s, monkeypatch, ea.Options(do_alpha=1e9), **how)
    assert (d1 == want).all(), (tag, np.flatnonzero(d1 != want)[:8])
    assert (d0 == want).all(), (tag, np.flatnonzero(d0 != want)[:8])
    assert key(st1) == key(st0), (tag, key(st1), key(st0))
    assert st0.pull_iterations == 0, tag
    if must_pull:
        assert st1.pull_iterations > 0, tag
    return st1


def host(g):
    Ap, Aj, _ = g.to_host()
    return Ap, np.ascontiguousarray(Aj[: g.nnz])


def make_known_symmetric(ea, ctx, g):
    """One direction-optimised call verifies on the device that the CSR is its own transpose."""
    ea.bfs(ctx, g, 0, options=ea.Options(direction_optimized=True))
    return g


def csr_of_rows(rows):
    Ap = np.zeros(len(rows) + 1, np.int32)
    Ap[1:] = np.cumsum([len(r) for r in rows])
    Aj = np.array([c for r in rows for c in r], np.int32)
    return Ap, Aj, np.ones(len(Aj), np.float32)


def test_chesapeake_every_source(gpu, oracle, monkeypatch):
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    g = ea.Graph.from_mtx(os.path.join(GOLDEN_DIR, "chesapeake.mtx"))
    Ap, Aj = host(g)
    assert g.n_rows == 39
    for s in range(g.n_rows):
        want, _ = oracle.bfs_heap(Ap, Aj, s)
        check_pulled(("chesapeake", s), ea, ctx, g, s, want, monkeypatch)
    g.close()


@functools.lru_cache(maxsize=4)
def rmat_wanted(oracle, scale):
    n, Ap, Aj, _ = oracle.rmat_csr(scale, 16, 1, 7, True)
    Aj = np.ascontiguousarray(Aj)
    rng = np.random.default_rng(1000 + scale)
    sources = [0, int(np.argmax(np.diff(Ap)))] + [int(x) for x in rng.integers(0, n, 3)]
    return Ap, Aj, {s: oracle.bfs_heap(Ap, Aj, s)[0] for s in sources}


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_rmat_symmetric(gpu, oracle, monkeypatch, scale):
    """Caller's numbering and hot-first copy, 4-byte and byte labels."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    Ap, Aj, wanted = rmat_wanted(oracle, scale)
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    gAp, gAj = host(g)
    assert (gAp == Ap).all() and (gAj == Aj).all()
    for hot in (False, True):
        g.hot_first(ctx, hot)
        for byte_labels in (False, True):
            for s, want in wanted.items():
                # an isolated source ends after level 0: nothing with a work hint, nothing pulled
                st = check_pulled((scale, hot, byte_labels, s), ea, ctx, g, s, want, monkeypatch,
                                  must_pull=Ap[s + 1] > Ap[s], byte_labels=byte_labels)
                if Ap[s + 1] > Ap[s]:   # every level after the first has a work hint and pulls
                    assert st.pull_iterations == st.iterations - 1, (scale, hot, s, st)
    g.close()


ROW_LENGTHS = (1, 16, 17, 64, 65, 1000)


def last_entry_graph():
    """0 - p; for every length L a vertex x whose row is L - 1 leaves of its own and then p, LAST: at
    the level whose frontier is {p} x finds its only frontier neighbour at the end of its row (probe
    limit 16, hand-over to the wavefront walk, its steps of 64 and ballot exit).  A vertex without a
    row, and an unreachable component (a hub of 100 spokes with a tail of 20) that walks its whole
    rows at every pulled level."""
    rows = [[1], [0]]            # 0: source, 1: p
    xs = []
    for L in ROW_LENGTHS:
        x = len(rows)
        xs.append(x)
        rows.append(None)
        leaves = list(range(len(rows), len(rows) + L - 1))
        rows += [[x] for _ in leaves]
        rows[x] = leaves + [1]
        rows[1].append(x)
    lonely = len(rows)
    rows.append([])
    hub = len(rows)
    rows.append([])
    for _ in range(100):
        rows.append([hub])
        rows[hub].append(len(rows) - 1)
    prev = hub
    for _ in range(20):
        rows.append([prev])
        rows[prev].append(len(rows) - 1)
        prev = len(rows) - 1
    return csr_of_rows(rows), xs, lonely, hub


@pytest.mark.parametrize("hot", [False, True])
def test_only_frontier_neighbour_is_last_in_row(gpu, oracle, monkeypatch, hot):
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    (Ap, Aj, Ax), xs, lonely, hub = last_entry_graph()
    assert [Ap[x + 1] - Ap[x] for x in xs] == list(ROW_LENGTHS) and all(Aj[Ap[x + 1] - 1] == 1 for x in xs)
    g = make_known_symmetric(ea, ctx, ea.Graph.from_host_csr(Ap, Aj, Ax))
    g.hot_first(ctx, hot)
    want, _ = oracle.bfs_heap(Ap, Aj, 0)
    assert (want[xs] == 2).all() and want[lonely] == INF_I and (want[hub:] == INF_I).all()
    for byte_labels in (False, True):
        st = check_pulled((hot, byte_labels), ea, ctx, g, 0, want, monkeypatch, byte_labels=byte_labels)
        assert st.iterations == 4 and st.pull_iterations == 3, st   # levels {p}, {x}, {leaves} pull
    # ... and from inside the other component: the hub's 101 entries, none in the frontier but the last
    want, _ = oracle.bfs_heap(Ap, Aj, len(Ap) - 2)
    check_pulled((hot, "tail"), ea, ctx, g, len(Ap) - 2, want, monkeypatch)
    g.close()


def test_path_across_the_byte_label_switch(gpu, oracle, monkeypatch):
    """300 vertices in a line: every level after the first pulls, byte labels until level 254 and the
    4-byte array from level 255 on."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n = 300
    rows = [[v + d for d in (-1, 1) if 0 <= v + d < n] for v in range(n)]
    Ap, Aj, Ax = csr_of_rows(rows)
    g = make_known_symmetric(ea, ctx, ea.Graph.from_host_csr(Ap, Aj, Ax))
    want, _ = oracle.bfs_heap(Ap, Aj, 0)
    assert want[-1] == n - 1
    for byte_labels in (True, False):
        st = check_pulled(("path", byte_labels), ea, ctx, g, 0, want, monkeypatch, byte_labels=byte_labels)
        assert st.iterations == n and st.pull_iterations == n - 1, st
    g.close()


@pytest.mark.parametrize("n", [1, 2, 63, 65, 4097])
def test_vertex_counts(gpu, oracle, monkeypatch, n):
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    rng = np.random.default_rng(77 + n)
    m = max(1, 3 * n)
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    a[0], b[0] = 0, n - 1                      # 0 has a neighbour (itself when n == 1)
    pairs = np.unique(np.concatenate([np.stack([a, b], 1), np.stack([b, a], 1)]), axis=0)
    rows = [[] for _ in range(n)]
    for u, v in pairs[rng.permutation(len(pairs))]:   # rows in no particular order
        rows[u].append(int(v))
    Ap, Aj, Ax = csr_of_rows(rows)
    g = make_known_symmetric(ea, ctx, ea.Graph.from_host_csr(Ap, Aj, Ax))
    for s in sorted({0, n - 1, n // 2}):
        want, _ = oracle.bfs_heap(Ap, Aj, s)
        # n == 1: the search ends after level 0, which has no work hint and never pulls
        check_pulled((n, s), ea, ctx, g, s, want, monkeypatch, must_pull=bool((want[want != INF_I] > 0).any()))
    g.close()


def test_rmat20_default_thresholds_and_options(gpu, oracle, monkeypatch):
    """1 M vertices: more than the 786,432 ids the settled image covers."""
    ea = gpu
    ctx = ea.Context(0)
    g = ea.Graph.rmat(ctx, 20, 16, 1, 7)
    assert g.n_rows > 786432
    Ap, Aj = host(g)
    want, _ = oracle.bfs_heap(Ap, Aj, 0)
    (d1, st1), (d0, st0) = run(ea, ctx, g, 0, monkeypatch, None)
    assert (d1 == want).all() and (d0 == want).all()
    assert st1.pull_iterations >= 1 and st0.pull_iterations == 0, (st1, st0)
    assert key(st1) == key(st0), (key(st1), key(st0))
    g.close()


def test_graphs_that_must_not_pull(gpu, oracle, monkeypatch):
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    force = ea.Options(do_alpha=1e9)
    monkeypatch.setenv("GRX_BFS_PULL", "1")

    def never(tag, g, options):
        Ap, Aj = host(g)
        for s in (0, int(np.argmax(np.diff(Ap)))):
            d, st = ea.bfs(ctx, g, s, options=options)
            want, _ = oracle.bfs_heap(Ap, Aj, s)
            assert (d.cpu().numpy() == want).all(), (tag, s)
            assert st.pull_iterations == 0 and st.iterations > 2, (tag, s, st)

    sym = ea.Graph.rmat(ctx, 12, 16, 1, 7)
    Ap, Aj, Ax = sym.to_host()
    unknown = ea.Graph.from_host_csr(Ap, Aj[: sym.nnz], Ax[: sym.nnz])   # symmetric, but nobody has said so
    never("symmetry unknown", unknown, force)
    never("alpha forbids", sym, ea.Options(do_alpha=1e-9))
    directed = ea.Graph.rmat(ctx, 12, 16, 1, 7, symmetrize=False)
    never("asymmetric", directed, force)
    directed.build_in_edges(ctx)
    never("asymmetric with in-edges", directed, force)
    for g in (sym, unknown, directed):
        g.close()


def two_parts_behind_a_bridge(oracle):
    """Two copies of symmetric RMAT-19 (1 M vertices together: more than the settled image covers) joined
    by a path of three from the vertex of part one that is farthest from its largest hub to the largest
    hub of part two.  Searched from part one's hub the work per level goes wide (part one), narrow (its
    tail, the path, the hub of part two alone), wide again (part two)."""
    n1, Ap1, Aj1, _ = oracle.rmat_csr(19, 16, 1, 7, True)
    Aj1 = np.ascontiguousarray(Aj1)
    hub = int(np.argmax(np.diff(Ap1)))
    d1, _ = oracle.bfs_heap(Ap1, Aj1, hub)
    a = int(np.argmax(np.where(d1 == INF_I, -1, d1)))
    b = n1 + hub
    path = [2 * n1, 2 * n1 + 1, 2 * n1 + 2]
    nnz1 = len(Aj1)
    Ap = np.concatenate([Ap1[:-1], Ap1 + nnz1]).astype(np.int64)
    Aj = np.insert(np.concatenate([Aj1, Aj1 + n1]), [Ap[a + 1], Ap[b + 1]], [path[0], path[-1]])
    Ap[a + 1:] += 1
    Ap[b + 1:] += 1
    rows = [[a, path[1]], [path[0], path[2]], [path[1], b]]
    Ap = np.concatenate([Ap, Ap[-1] + np.cumsum([len(r) for r in rows])]).astype(np.int32)
    Aj = np.concatenate([Aj, np.array(sum(rows, []), Aj.dtype)]).astype(np.int32)
    return Ap, Aj, hub


def test_wide_narrow_wide_with_default_thresholds(gpu, oracle, monkeypatch):
    """A label-scan level leaves the NEXT level's settled bits; narrow levels that follow run without a
    bitmap, and the next wide level must not take those old bits for its snapshot: every vertex labelled
    in between would be a frontier vertex without a bit, invisible to the neighbours that pull."""
    ea = gpu
    ctx = ea.Context(0)
    Ap, Aj, s = two_parts_behind_a_bridge(oracle)
    n, nnz, deg = len(Ap) - 1, len(Aj), np.diff(Ap)
    assert n >= 786432
    want, _ = oracle.bfs_heap(Ap, Aj, s)
    work = np.bincount(want[want != INF_I], weights=deg[want != INF_I]).astype(np.int64)
    # the rule of bfs_enactor_t with its defaults: a level of >= 1 M edges refreshes the bitmap, one of
    # >= 2 M scans the labels, and a scanning level pulls when work > (nnz - work of levels 1..l) / 16
    kinds, logged = ["narrow"], 0
    for l in range(1, len(work)):
        logged += int(work[l])
        scan = work[l] >= 2 << 20
        kinds.append("pull" if scan and work[l] > (nnz - logged) / 16 else "scan" if scan else
                     "wide" if work[l] >= 1 << 20 else "narrow")
    first = min(l for l, k in enumerate(kinds) if k in ("pull", "scan"))
    gap = min(l for l, k in enumerate(kinds) if l > first and k == "narrow")
    again = [l for l, k in enumerate(kinds) if l > gap and k == "pull"]
    assert again, kinds                           # a pulled level behind narrow levels behind a scan
    g = make_known_symmetric(ea, ctx, ea.Graph.from_host_csr(Ap, Aj, np.ones(nnz, np.float32)))
    for hot in (False, True):
        g.hot_first(ctx, hot)
        (d1, st1), (d0, st0) = run(ea, ctx, g, s, monkeypatch, None)
        assert (d0 == want).all(), hot
        assert (d1 == want).all(), (hot, kinds, int((d1 != want).sum()))
        assert key(st1) == key(st0), (hot, key(st1), key(st0))
        assert st1.pull_iterations == kinds.count("pull") and st0.pull_iterations == 0, (hot, st1, kinds)
    g.close()
