"""Near / far selection of grx_sssp (sssp_enactor_t::select_near): a wide pending
set is expanded nearest share first, the rest waits while its labels fall.

Reference: oracle.sssp_heap (float32 Dijkstra), compared bit for bit, for the reason
tests/test_gpu_sssp_wide.py derives: both are the minimum over all paths of the left-to-right float32
path sums, whatever the order of the relaxations.  Deferral changes only that order.

Every run is witnessed through GRX_DEBUG: next to the `[grx] sssp iteration` line of every iteration
the selection prints `[grx] sssp near: iteration i threshold T near_work a deferred_work b`.  A forced
run (GRX_SSSP_NEAR_MIN_WORK=1) must defer at least once, must scan while deferred work remains and
must end with nothing deferred.
"""
import functools
import os
import re

import numpy as np
import pytest

from sssp_families import FLT_MAX, inexact_share, weights

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

FORM = re.compile(r"\[grx\] sssp iteration (\d+): form (\w) scan (\d) snapshot (\d) slots (\d+) work (-?\d+)")
NEAR = re.compile(r"\[grx\] sssp near: iteration (\d+) threshold (\d+) near_work (\d+) deferred_work (\d+)")
FORCED = {"GRX_SSSP_NEAR_MIN_WORK": "1", "GRX_SETTLED_MIN_WORK": "1", "GRX_LABEL_SCAN_MIN_WORK": "1"}
PER_CALL = ("GRX_SSSP_NEAR", "GRX_SSSP_NEAR_FRAC", "GRX_SSSP_EARLY_LIVE", "GRX_SSSP_PACKED",
            "GRX_SSSP_BOUND_FROM")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sssp_near_off_lines.txt")


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


@functools.lru_cache(maxsize=2)
def rmat(oracle, scale, symmetric):
    n, Ap, Aj, Ax = oracle.rmat_csr(scale, 16, 1, 7, symmetric)
    return n, Ap, np.ascontiguousarray(Aj), np.ascontiguousarray(Ax)


def induced(Ap, Aj, Ax, n):
    """The subgraph on the vertices below n."""
    rows = np.repeat(np.arange(len(Ap) - 1, dtype=np.int64), np.diff(Ap))
    keep = (rows < n) & (Aj < n)
    out = np.zeros(n + 1, np.int64)
    np.add.at(out, rows[keep] + 1, 1)
    return np.cumsum(out).astype(np.int32), np.ascontiguousarray(Aj[keep]), np.ascontiguousarray(Ax[keep])


def run(ea, ctx, G, s, capfd):
    """-> (distances, Stats, iteration lines [(form, scan, work)], near lines [(iteration, threshold,
    near_work, deferred_work)], the raw iteration lines, both kinds of line in the order printed)."""
    capfd.readouterr()
    d, st = ea.sssp(ctx, G, int(s))
    got = d.cpu().numpy()
    forms, near, raw, events = [], [], [], []
    for line in capfd.readouterr().err.splitlines():
        m = FORM.search(line)
        if m:
            assert int(m.group(1)) == len(forms), line
            forms.append((m.group(2), int(m.group(3)), int(m.group(6))))
            raw.append(m.group(0))
            events.append(("form",) + forms[-1])
        m = NEAR.search(line)
        if m:
            near.append(tuple(int(x) for x in m.groups()))
            events.append(("near",) + near[-1])
    assert forms
    return got, st, forms, near, raw, events


def check(tag, got, st, want, deg):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (tag, f"{bad.size} of {len(want)} distances differ", bad[:5].tolist(),
                           got[bad[:5]].tolist(), want[bad[:5]].tolist())
    reached = want != FLT_MAX
    assert st.vertices_reached == int(reached.sum()), tag
    assert st.edges_traversed == int(deg[reached].sum()), tag
    assert st.edges_expanded >= st.edges_traversed, tag


def check_deferral(tag, events, expect_deferred):
    """What the debug lines of a forced run must say: it defers (where there is enough to split), an
    iteration that runs while work is deferred scans, a round never takes nothing and leaves
    something, and nothing is deferred when the run ends."""
    deferred, ever = 0, False
    for e in events:
        if e[0] == "near":
            _, _, _, near_work, deferred = e
            assert near_work > 0 or deferred == 0, (tag, events)
            ever = ever or deferred > 0
        elif deferred > 0:
            assert e[2] == 1 and e[1] in "BDE", (tag, e, events)
    assert deferred == 0, (tag, events)
    if expect_deferred:
        assert ever, (tag, events)
    return ever


def pick_sources(deg, rng):
    """0, a vertex of degree 1 and a seeded random one with edges."""
    ones = np.flatnonzero(deg == 1)
    assert ones.size, "no degree-1 vertex"
    others = np.flatnonzero(deg > 1)
    others = others[others != 0]
    return [0, int(rng.choice(ones)), int(rng.choice(others))]


def forced_case(ea, oracle, capfd, monkeypatch, tag, Ap, Aj, Ax, sources, want=None):
    ctx = forced_context(ea, monkeypatch)
    deg = np.diff(Ap)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    want = want or {s: oracle.sssp_heap(Ap, Aj, Ax, int(s))[0] for s in sources}
    deferred_somewhere = False
    for hot in (True, False):
        G.hot_first(ctx, hot)
        for early in (0, 1):
            for s in sources:
                per_call(monkeypatch, GRX_SSSP_EARLY_LIVE=early)
                got, st, forms, near, _, events = run(ea, ctx, G, s, capfd)
                t = (tag, hot, early, s, "".join(f[0] for f in forms))
                check(t, got, st, want[s], deg)
                wide = (want[s] != FLT_MAX).sum() > 64      # a source in a tiny component may defer nothing
                deferred_somewhere |= check_deferral(t, events, expect_deferred=wide)
    assert deferred_somewhere, tag
    G.close()
    return want


@pytest.mark.parametrize("scale", [12, 14, 16])
def test_forced_on_symmetric_rmat(gpu, oracle, capfd, monkeypatch, scale):
    """Deferral forced from one edge of pending work on, on symmetric R-MAT with the bench's weights
    (1..64), hot-first numbering on and off, GRX_SSSP_EARLY_LIVE 0 and 1, three sources."""
    n, Ap, Aj, Ax = rmat(oracle, scale, True)
    sources = pick_sources(np.diff(Ap), np.random.default_rng(scale))
    forced_case(gpu, oracle, capfd, monkeypatch, ("rmat", scale), Ap, Aj, Ax, sources)


@pytest.mark.parametrize("n", [4097, 49151, 49152, 49153, 60001])
def test_forced_on_odd_sizes(gpu, oracle, capfd, monkeypatch, n):
    """Sizes around the 49,152 ids of the LDS bound image and sizes that are no multiple of 8: the
    subgraph of symmetric R-MAT-16 on the ids below n."""
    _, Ap, Aj, Ax = rmat(oracle, 16, True)
    Ap, Aj, Ax = induced(Ap, Aj, Ax, n)
    sources = pick_sources(np.diff(Ap), np.random.default_rng(n))
    forced_case(gpu, oracle, capfd, monkeypatch, ("odd", n), Ap, Aj, Ax, sources)


def test_forced_inexact_float_sums(gpu, oracle, capfd, monkeypatch):
    """Fractional weights: nearly every distance has non-zero low 16 bits, so the histogram's code
    and the 2-byte bound are both inexact images of it."""
    _, Ap, Aj, _ = rmat(oracle, 16, True)
    Ax = weights("frac", Ap, Aj, 16, True)
    sources = pick_sources(np.diff(Ap), np.random.default_rng(3))
    want = {s: oracle.sssp_heap(Ap, Aj, Ax, int(s))[0] for s in sources}
    for s in sources:
        assert inexact_share(want[s], int(s)) >= 0.99, s
    forced_case(gpu, oracle, capfd, monkeypatch, "frac", Ap, Aj, Ax, sources, want)


def test_forced_directed_with_sinks(gpu, oracle, capfd, monkeypatch):
    """Directed R-MAT-16: sinks (in-edges only) lie beyond leading_connected on the hot-first copy.
    They are never pending and never expanded, and must get the oracle's labels all the same."""
    ea = gpu
    n, Ap, Aj, Ax = rmat(oracle, 16, False)
    deg = np.diff(Ap)
    sinks = (deg == 0) & (np.bincount(Aj, minlength=n) > 0)
    assert sinks.sum() > 1000
    rng = np.random.default_rng(16)
    heavy = np.flatnonzero(deg > 64)
    sources = [0, int(rng.choice(heavy)), int(rng.choice(heavy))]
    want = forced_case(ea, oracle, capfd, monkeypatch, "directed", Ap, Aj, Ax, sources)
    ctx = forced_context(ea, monkeypatch)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    G.hot_first(ctx, True)
    for s in sources:
        per_call(monkeypatch)
        got, st, forms, near, _, _ = run(ea, ctx, G, s, capfd)
        assert (got[sinks].view(np.uint32) == want[s][sinks].view(np.uint32)).all(), s
        assert (want[s][sinks] != FLT_MAX).sum() > 1000 or s != 0
    G.close()


def star_plus_path(leaves=3000, path=40):
    """0 -- 1..leaves (a star), and a path leaves -- leaves+1 -- ... of `path` more vertices; undirected,
    unit weights.  Every frontier is one distance: {0}, the leaves, then one path vertex per round."""
    rows, cols = [], []
    for v in range(1, leaves + 1):
        rows += [0, v]; cols += [v, 0]
    for v in range(leaves, leaves + path):
        rows += [v, v + 1]; cols += [v + 1, v]
    n = leaves + path + 1
    order = np.lexsort((cols, rows))
    rows = np.array(rows, np.int32)[order]
    Ap = np.zeros(n + 1, np.int32)
    np.add.at(Ap, rows + 1, 1)
    return np.cumsum(Ap).astype(np.int32), np.ascontiguousarray(np.array(cols, np.int32)[order]), \
        np.ones(len(rows), np.float32)


def test_all_distances_equal(gpu, oracle, capfd, monkeypatch):
    """Every pending vertex falls into ONE histogram bin: the threshold must take them all (a share
    of one bin cannot be taken) and the run must terminate with the oracle's labels."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    Ap, Aj, Ax = star_plus_path()
    deg = np.diff(Ap)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    for hot in (True, False):
        G.hot_first(ctx, hot)
        per_call(monkeypatch)
        got, st, forms, near, _, _ = run(ea, ctx, G, 0, capfd)
        check(("star", hot), got, st, want, deg)
        assert near and all(n[3] == 0 for n in near), near       # one bin: nothing can be deferred
        assert st.edges_expanded == st.edges_traversed           # every vertex expanded exactly once
    G.close()


def switch_off_lines(ea, ctx, capfd, monkeypatch):
    """The iteration lines of the runs the golden file records, deferral switched off."""
    lines = []
    Ap, Aj, Ax = star_plus_path()
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    for hot in (True, False):
        G.hot_first(ctx, hot)
        for early in (0, 1):
            per_call(monkeypatch, GRX_SSSP_NEAR=0, GRX_SSSP_EARLY_LIVE=early)
            _, _, _, near, raw, _ = run(ea, ctx, G, 0, capfd)
            assert not near
            lines += [f"hot {int(hot)} early {early} {l}" for l in raw]
    G.close()
    return lines


def test_switch_off_prints_the_parents_lines(gpu, oracle, capfd, monkeypatch):
    """GRX_SSSP_NEAR=0: no selection line, and the iteration lines are those the commit before
    deferral printed for the same calls (tests/golden/sssp_near_off_lines.txt, recorded with that
    commit's library on a graph whose frontiers do not depend on timing: star_plus_path), with every
    threshold forced to 1.  On R-MAT, where frontiers do depend on timing, the forms must still be the
    ones the thresholds alone decide."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    with open(GOLDEN) as f:
        recorded = [l.rstrip("\n") for l in f if l.strip()]
    assert switch_off_lines(ea, ctx, capfd, monkeypatch) == recorded
    n, Ap, Aj, Ax = rmat(oracle, 14, True)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    per_call(monkeypatch, GRX_SSSP_NEAR=0)
    got, st, forms, near, _, _ = run(ea, ctx, G, 0, capfd)
    check("off", got, st, oracle.sssp_heap(Ap, Aj, Ax, 0)[0], np.diff(Ap))
    assert not near
    assert forms[0][0] == "A" and all(f[0] in "BDE" and f[1] == 1 for f in forms[1:] if f[2] > 0), forms
    G.close()


def test_fewer_relaxations(gpu, oracle, capfd, monkeypatch):
    """Symmetric R-MAT-16, source 0, forced: deferral must expand strictly fewer edges than the same
    call with GRX_SSSP_NEAR=0 (the synchronous simulation, tools/sssp_near_sim.py, gives 0.65 - 0.68
    at scale 18; the measured ratio is printed and recorded in profiles/sssp_near_ab.txt)."""
    ea = gpu
    ctx = forced_context(ea, monkeypatch)
    n, Ap, Aj, Ax = rmat(oracle, 16, True)
    deg = np.diff(Ap)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    expanded = {}
    for on in (1, 0):
        per_call(monkeypatch, GRX_SSSP_NEAR=on)
        got, st, forms, near, _, _ = run(ea, ctx, G, 0, capfd)
        check(("fewer", on), got, st, want, deg)
        assert bool(near) == bool(on)
        expanded[on] = (st.edges_expanded, st.iterations)
    print(f"[sssp near] rmat16 source 0 forced: edges_expanded {expanded[1][0]} with deferral "
          f"({expanded[1][1]} iterations), {expanded[0][0]} without ({expanded[0][1]}), ratio "
          f"{expanded[1][0] / expanded[0][0]:.3f}, reached edges {st.edges_traversed}")
    assert expanded[1][0] < expanded[0][0], expanded
    G.close()
