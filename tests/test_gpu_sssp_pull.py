"""Pulled rounds of grx_sssp (sssp_enactor_t::pull_round): on a graph KNOWN to be
its own transpose with equal weights a scanning wide round is pulled over rows sorted by ascending
weight, every row left where fl(dmin + w) reaches the label of its vertex.

Reference: oracle.sssp_heap (float32 Dijkstra), compared bit for bit, for the reason
tests/test_gpu_sssp_wide.py derives: both are the minimum over all paths of the left-to-right float32
path sums, whatever the order of the relaxations.  A pulled round changes which relaxations are made
at all; the ones it leaves out are provably not shorter (float addition is monotone in each argument).

Every run is witnessed through GRX_DEBUG: a pulled round prints `form P scan 1 snapshot 0` in its
iteration line and `[grx] sssp pull: iteration i dmin D examined E unreached_work U`.  The graphs
come from the two builders that vouch for equal weights: Graph.rmat(symmetrize=True) and a symmetric
Matrix Market file (weights printed with 9 significant digits, which float32 survives).
"""
import functools
import os
import re

import numpy as np
import pytest

from sssp_families import FLT_MAX, INEXACT, inexact_share, weights

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

FORM = re.compile(r"\[grx\] sssp iteration (\d+): form (\w) scan (\d) snapshot (\d) slots (\d+) work (-?\d+)")
PULL = re.compile(r"\[grx\] sssp pull: iteration (\d+) dmin (\S+) examined (\d+) unreached_work (\d+)")
FORCED = {"GRX_SSSP_NEAR_MIN_WORK": "1", "GRX_SETTLED_MIN_WORK": "1", "GRX_LABEL_SCAN_MIN_WORK": "1"}
PER_CALL = ("GRX_SSSP_PULL", "GRX_SSSP_PULL_ALPHA", "GRX_SSSP_NEAR", "GRX_SSSP_NEAR_FRAC", "GRX_SSSP_EARLY_LIVE",
            "GRX_SSSP_PACKED", "GRX_SSSP_BOUND_FROM")


def probe_length():
    """SSSP_PULL_PROBES as the kernel's header has it: the entries a lane reads before the wavefront
    takes over.  Read, not repeated, so that the boundary cases move with the constant."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gunrock", "hip",
                          "kernels", "advance_kernels.hxx")
    with open(header) as f:
        m = re.search(r"constexpr int SSSP_PULL_PROBES = (\d+);", f.read())
    assert m, "SSSP_PULL_PROBES not found in advance_kernels.hxx"
    return int(m.group(1))


PROBES = probe_length()


@pytest.fixture
def gpu(oracle, monkeypatch):
    import torch
    import essentials_amd as ea
    assert torch.cuda.is_available()
    monkeypatch.setenv("GRX_DEBUG", "1")
    for name in PER_CALL + tuple(FORCED) + ("GRX_FUSED_MIN_SLOTS", "GRX_HOT_FIRST"):
        monkeypatch.delenv(name, raising=False)
    return ea


def forced_context(ea, monkeypatch):
    """The thresholds are read when a context is made."""
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    return ea.Context(0)


def per_call(monkeypatch, **env):
    for name in PER_CALL:
        if env.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(env[name]))


def run(ea, ctx, G, s, capfd):
    """-> (distances, Stats, [(form, scan, snapshot, work)] per iteration, [(iteration, examined,
    unreached_work)] per pulled round)."""
    capfd.readouterr()
    d, st = ea.sssp(ctx, G, int(s))
    got = d.cpu().numpy()
    forms, pulls = [], []
    for line in capfd.readouterr().err.splitlines():
        m = FORM.search(line)
        if m:
            assert int(m.group(1)) == len(forms), line
            forms.append((m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(6))))
        m = PULL.search(line)
        if m:
            pulls.append((int(m.group(1)), int(m.group(3)), int(m.group(4))))
    assert forms
    return got, st, forms, pulls


def check(tag, got, st, want, deg):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (tag, f"{bad.size} of {len(want)} distances differ", bad[:5].tolist(),
                           got[bad[:5]].tolist(), want[bad[:5]].tolist())
    reached = want != FLT_MAX
    assert st.vertices_reached == int(reached.sum()), tag
    assert st.edges_traversed == int(deg[reached].sum()), tag
    assert st.edges_expanded >= st.edges_traversed, tag


def check_pulled(tag, forms, pulls):
    """A pulled round is a scanning round without a snapshot, and prints its own line."""
    p = [i for i, f in enumerate(forms) if f[0] == "P"]
    assert p, (tag, forms)
    assert all(forms[i][1:3] == (1, 0) for i in p), (tag, forms)
    assert [q[0] for q in pulls] == p, (tag, forms, pulls)


def symmetric_mtx(path, n, rows, cols, vals):
    """A symmetric Matrix Market file of the undirected edges (rows[i], cols[i]) with weight vals[i]."""
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{n} {n} {len(rows)}\n")
        for r, c, w in zip(rows, cols, vals):
            hi, lo = (r, c) if r >= c else (c, r)
            f.write(f"{hi + 1} {lo + 1} {np.float32(w):.9g}\n")
    return str(path)


def lower_triangle(Ap, Aj, Ax):
    """The entries (r, c) with c <= r of a symmetric CSR: every undirected edge once (repeats kept)."""
    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))
    keep = Aj <= rows
    return rows[keep], Aj[keep], Ax[keep]


def from_file(ea, tmp_path, n, rows, cols, vals, name="g.mtx"):
    """-> (Graph loaded from a symmetric file, its CSR as the library holds it)."""
    G = ea.Graph.from_mtx(symmetric_mtx(tmp_path / name, n, rows, cols, vals))
    Ap, Aj, Ax = G.to_host()
    assert G.n_rows == n
    return G, Ap, np.ascontiguousarray(Aj), np.ascontiguousarray(Ax)


def seeded_sources(deg, seed, count=3):
    rng = np.random.default_rng(seed)
    others = np.flatnonzero(deg > 0)
    others = others[others != 0]
    return [0] + [int(x) for x in rng.choice(others, count, replace=False)]


@functools.lru_cache(maxsize=4)
def rmat(oracle, scale, symmetric=True, edge_factor=16, seed=1):
    n, Ap, Aj, Ax = oracle.rmat_csr(scale, edge_factor, seed, 7, symmetric)
    return n, Ap, np.ascontiguousarray(Aj), np.ascontiguousarray(Ax)


def forced_runs(ea, ctx, oracle, capfd, monkeypatch, tag, G, Ap, Aj, Ax, sources, alpha=0):
    """Every source with pulling forced (alpha 0): exact distances and stats, a pulled round wherever
    the source reaches more than a handful of vertices.  -> {source: (forms, pulls, distances)}."""
    deg = np.diff(Ap)
    G.hot_first(ctx, True)
    out = {}
    for s in sources:
        want, _ = oracle.sssp_heap(Ap, Aj, Ax, int(s))
        per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=alpha)
        got, st, forms, pulls = run(ea, ctx, G, s, capfd)
        check((tag, s, "".join(f[0] for f in forms)), got, st, want, deg)
        if (want != FLT_MAX).sum() > 64:
            check_pulled((tag, s), forms, pulls)
        out[s] = (forms, pulls, want)
    # whatever the components of the seeded sources: no case passes without a witnessed pulled round
    assert any(f[0] == "P" for forms, _, _ in out.values() for f in forms), (tag, sources)
    return out


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_rmat(gpu, oracle, capfd, monkeypatch, scale):
    """Graph.rmat with the bench's weights (1..64, weight seed 7): repeats and self loops included."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    G = ea.Graph.rmat(ctx, scale, 16, seed=1, weight_seed=7, symmetrize=True)
    Ap, Aj, Ax = G.to_host()
    rows = np.repeat(np.arange(G.n_rows), np.diff(Ap))
    assert (Aj == rows).any() and len(Aj) > len(np.unique(rows.astype(np.int64) * G.n_rows + Aj))
    forced_runs(ea, ctx, oracle, capfd, monkeypatch, ("rmat", scale), G, Ap, Aj, Ax,
                seeded_sources(np.diff(Ap), scale))
    G.close()


@pytest.mark.parametrize("family", INEXACT)
def test_inexact_sums(gpu, oracle, capfd, monkeypatch, tmp_path, family):
    """Weights whose float32 path sums round: fl(dmin + w) and fl(d(u) + w) are both inexact, and the
    cut-off must still never skip an entry that carries a shorter path."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n, Ap0, Aj0, _ = rmat(oracle, 12)
    G, Ap, Aj, Ax = from_file(ea, tmp_path, n, *lower_triangle(Ap0, Aj0, weights(family, Ap0, Aj0, 16, True)))
    assert len(Aj) == len(Aj0)
    sources = seeded_sources(np.diff(Ap), 12, 2)
    out = forced_runs(ea, ctx, oracle, capfd, monkeypatch, family, G, Ap, Aj, Ax, sources)
    assert inexact_share(out[0][2], 0) >= 0.99
    G.close()


@pytest.mark.parametrize("kind", ["ones", "zeros"])
def test_ties_and_zeros(gpu, oracle, capfd, monkeypatch, tmp_path, kind):
    """All weights 1.0 (every row is one long tie, every frontier one distance), and a fifth of the
    edges 0.0 (fl(dmin + 0) == dmin: the test is strict, an equal distance is not an improvement)."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n, Ap0, Aj0, _ = rmat(oracle, 12)
    W = np.ones(len(Aj0), np.float32) if kind == "ones" else weights("zeros", Ap0, Aj0, 5, True)
    G, Ap, Aj, Ax = from_file(ea, tmp_path, n, *lower_triangle(Ap0, Aj0, W))
    assert kind == "ones" or (Ax == 0).mean() > 0.15
    forced_runs(ea, ctx, oracle, capfd, monkeypatch, kind, G, Ap, Aj, Ax, seeded_sources(np.diff(Ap), 3, 2))
    G.close()


def long_row_graph(length):
    """0 -(1)- 1 -(100)- 2, and 2 -(0.5 i)- 2 + i for i = 1 .. length - 1: the row of vertex 2 has
    `length` entries, its HEAVIEST leads to the only neighbour the source reaches first, so vertex 2
    must read its whole row in the round that reaches it; its leaves hang on it alone.  A few more
    neighbours of 0 and 1 make the first frontiers more than one vertex."""
    rows, cols, vals = [0, 1], [1, 2], [1.0, 100.0]
    for i in range(1, length):
        rows.append(2); cols.append(2 + i); vals.append(0.5 * i)
    n = 2 + length
    for k in range(5):   # 0 and 1 get five leaves each
        rows += [0, 1]; cols += [n + 2 * k, n + 2 * k + 1]; vals += [2.0 + k, 3.0 + k]
    return n + 10, rows, cols, vals


@pytest.mark.parametrize("length", [PROBES - 1, PROBES, PROBES + 1, PROBES + 63, PROBES + 64, PROBES + 65])
def test_row_length_boundaries(gpu, oracle, capfd, monkeypatch, tmp_path, length):
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n, rows, cols, vals = long_row_graph(length)
    G, Ap, Aj, Ax = from_file(ea, tmp_path, n, rows, cols, vals)
    assert np.diff(Ap)[2] == length and Ax[Ap[2]:Ap[3]].max() == 100.0
    G.hot_first(ctx, True)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    assert want[2] == 101.0 and (want != FLT_MAX).all()
    per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=0)
    got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
    check(("row", length), got, st, want, np.diff(Ap))
    check_pulled(("row", length), forms, pulls)
    assert max(p[1] for p in pulls) >= length, pulls   # the round that reached vertex 2 read its whole row
    G.close()


def test_unreached_parts(gpu, oracle, capfd, monkeypatch, tmp_path):
    """A second component and ids without edges (beyond leading_connected on the hot-first copy) keep
    FLT_MAX, and their degrees never count as reached."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n0, Ap0, Aj0, Ax0 = rmat(oracle, 10)
    rows, cols, vals = lower_triangle(Ap0, Aj0, Ax0)
    k = 40   # a second component: a ring of k vertices with chords, then 100 ids without edges
    ring = np.arange(k)
    rows = np.concatenate((rows, n0 + ring, n0 + ring))
    cols = np.concatenate((cols, n0 + (ring + 1) % k, n0 + (ring + 7) % k))
    vals = np.concatenate((vals, 1.0 + ring % 5, 2.0 + ring % 3)).astype(np.float32)
    n = n0 + k + 100
    G, Ap, Aj, Ax = from_file(ea, tmp_path, n, rows, cols, vals)
    deg = np.diff(Ap)
    assert (deg[n0 + k:] == 0).all() and (deg[n0:n0 + k] > 0).all()
    out = forced_runs(ea, ctx, oracle, capfd, monkeypatch, "parts", G, Ap, Aj, Ax, [0, n0 + 3])
    assert (out[0][2][n0:] == FLT_MAX).all() and (out[n0 + 3][2][:n0] == FLT_MAX).all()
    G.close()


def two_parts(oracle):
    """R-MAT-10 (edge factor 16) on the ids below 1024, a path of 6 vertices from the vertex of it that
    lies farthest from vertex 0 to vertex 0 of a second, sparser R-MAT-10 (edge factor 2, seed 2)
    behind it.  From source 0 the first part's wide rounds exceed everything still unreached (the
    second part is an eighth of the first), the path and the first part's tail are narrow, and the
    second part is wide against what is left."""
    n0, Ap0, Aj0, Ax0 = rmat(oracle, 10)
    n1, Ap1, Aj1, Ax1 = rmat(oracle, 10, True, 2, 2)
    r0, c0, v0 = lower_triangle(Ap0, Aj0, Ax0)
    r1, c1, v1 = lower_triangle(Ap1, Aj1, Ax1)
    d0, _ = oracle.sssp_heap(Ap0, Aj0, Ax0, 0)
    last = int(np.argmax(np.where(d0 != FLT_MAX, d0, -1)))
    hops = 6
    path = n0 + np.arange(hops)
    second = n0 + hops
    pr = np.concatenate(([last], path))
    pc = np.concatenate((path, [second]))
    rows = np.concatenate((r0, pr, r1 + second))
    cols = np.concatenate((c0, pc, c1 + second))
    vals = np.concatenate((v0, np.full(len(pr), 40.0, np.float32), v1)).astype(np.float32)
    return second + n1, rows, cols, vals, second


def test_mixed_rounds(gpu, oracle, capfd, monkeypatch, tmp_path):
    """Default alpha: pulled rounds, then push rounds, then pulled rounds again; distances exact."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n, rows, cols, vals, second = two_parts(oracle)
    G, Ap, Aj, Ax = from_file(ea, tmp_path, n, rows, cols, vals)
    G.hot_first(ctx, True)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    assert (want[second:] != FLT_MAX).sum() > 500
    per_call(monkeypatch)
    got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
    seq = "".join(f[0] for f in forms)
    check(("mixed", seq), got, st, want, np.diff(Ap))
    check_pulled(("mixed", seq), forms, pulls)
    assert re.search(r"P[^P]+P", seq), seq
    G.close()


def test_never_pulled(gpu, oracle, capfd, monkeypatch):
    """No verdict of equal weights, no pulled round -- and the same distances: the same arrays through
    from_host_csr, also after a direction-optimised BFS has verified their structural symmetry; a
    directed R-MAT; a structurally symmetric graph with unequal weights; GRX_SSSP_PULL=0."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    R = ea.Graph.rmat(ctx, 12, 16, seed=1, weight_seed=7, symmetrize=True)
    Ap, Aj, Ax = R.to_host()
    deg = np.diff(Ap)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)

    def expect_push(tag, G, Ap, Aj, Ax, want, **env):
        G.hot_first(ctx, True)
        per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=0, **env)
        got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
        check(tag, got, st, want, np.diff(Ap))
        assert not pulls and all(f[0] != "P" for f in forms), (tag, forms)
        assert any(f[0] in "BDE" and f[1] == 1 for f in forms), (tag, forms)   # the rounds a pull would take

    H = ea.Graph.from_host_csr(Ap, Aj, Ax)
    expect_push("from_host_csr", H, Ap, Aj, Ax, want)
    _, bfs_stats = ea.bfs(ctx, H, 0, options=ea.Options(direction_optimized=True))   # verifies the structure
    assert bfs_stats.vertices_reached == int((want != FLT_MAX).sum())
    expect_push("verified structure", H, Ap, Aj, Ax, want)
    H.close()

    D = ea.Graph.rmat(ctx, 12, 16, seed=1, weight_seed=7, symmetrize=False)
    dAp, dAj, dAx = D.to_host()
    expect_push("directed", D, dAp, dAj, dAx, oracle.sssp_heap(dAp, dAj, dAx, 0)[0])
    D.close()

    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))
    uneven = np.where(Aj < rows, Ax + np.float32(0.5), Ax).astype(np.float32)   # (u, v) and (v, u) differ
    U = ea.Graph.from_host_csr(Ap, Aj, uneven)
    expect_push("unequal weights", U, Ap, Aj, uneven, oracle.sssp_heap(Ap, Aj, uneven, 0)[0])
    U.close()

    expect_push("switched off", R, Ap, Aj, Ax, want, GRX_SSSP_PULL=0)
    per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=0)
    got, st, forms, pulls = run(ea, ctx, R, 0, capfd)   # the same handle does pull when allowed
    check("switched on", got, st, want, deg)
    check_pulled("switched on", forms, pulls)
    R.close()


def test_work_witness(gpu, oracle, capfd, monkeypatch):
    """R-MAT-14, every eligible round pulled: the entries the pulled rounds examine are at most the
    edges the same rounds would have pushed (the synchronous simulation, tools/sssp_pull_sim.py, gives
    about a tenth; the measured ratio is printed and recorded in profiles/sssp_pull_ab.txt)."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    G = ea.Graph.rmat(ctx, 14, 16, seed=1, weight_seed=7, symmetrize=True)
    Ap, Aj, Ax = G.to_host()
    out = forced_runs(ea, ctx, oracle, capfd, monkeypatch, "witness", G, Ap, Aj, Ax, [0])
    forms, pulls, _ = out[0]
    examined = sum(p[1] for p in pulls)
    work = sum(forms[p[0]][3] for p in pulls)
    print(f"[sssp pull] rmat14 source 0 forced: {len(pulls)} pulled rounds examined {examined} entries, "
          f"their frontiers hold {work} edges, ratio {examined / work:.3f}")
    assert examined <= work, (examined, work, forms, pulls)
    G.close()


def test_failed_build_pushes_and_is_tried_again(gpu, oracle, capfd, monkeypatch):
    """GRX_SSSP_PULL_BUILD_FAILS makes the build of the weight-sorted rows throw with its arrays
    allocated and nothing in them.  The call that asked must run as it did before there was anything to
    pull -- no error, no pulled round, exact distances -- the handle must keep nothing of the failed
    build, and the next call must build and pull."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    G = ea.Graph.rmat(ctx, 12, 16, seed=1, weight_seed=7, symmetrize=True)
    Ap, Aj, Ax = G.to_host()
    deg = np.diff(Ap)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    G.hot_first(ctx, True)
    for attempt in range(2):
        per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=0)
        monkeypatch.setenv("GRX_SSSP_PULL_BUILD_FAILS", "1")
        got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
        check(("failed build", attempt), got, st, want, deg)
        assert not pulls and all(f[0] != "P" for f in forms), forms
        assert st.pull_iterations == 0
    monkeypatch.delenv("GRX_SSSP_PULL_BUILD_FAILS")
    got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
    check("built after all", got, st, want, deg)
    check_pulled("built after all", forms, pulls)
    assert st.pull_iterations == len(pulls)
    G.close()


def test_attached_in_edges_withdraw_the_verdict(gpu, oracle, capfd, monkeypatch):
    """A handle that pulled stops pulling once in-edges are attached to it (the caller says: directed);
    distances stay exact."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    G = ea.Graph.rmat(ctx, 12, 16, seed=1, weight_seed=7, symmetrize=True)
    Ap, Aj, Ax = G.to_host()
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    G.hot_first(ctx, True)
    per_call(monkeypatch, GRX_SSSP_PULL_ALPHA=0)
    got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
    check("before", got, st, want, np.diff(Ap))
    check_pulled("before", forms, pulls)
    G.build_in_edges(ctx)
    got, st, forms, pulls = run(ea, ctx, G, 0, capfd)
    check("after", got, st, want, np.diff(Ap))
    assert not pulls and all(f[0] != "P" for f in forms), forms
    G.close()
