"""The wide-iteration forms of grx_sssp (sssp_enactor_t::loop) on weights for
which the 2-byte distance bound is INEXACT, on directed graphs with sinks, and forced onto small and
odd-sized graphs.

Reference: oracle.sssp_heap (float32 Dijkstra), compared bit for bit.  That is derived, not measured:
every candidate distance is one left-to-right float32 sum along a path, float addition is monotone in
its left operand and the weights are non-negative, so Dijkstra's result and the engine's fix point are
both the minimum of those sums over all paths.  A 1-ULP difference is a finding.

Every run is witnessed: with GRX_DEBUG set the enactor names the form of each iteration on stderr
(A plain, B label scan, C bounded, D bounded + scan, E early-live; whether snapshot_bounds ran), and
each case asserts that the forms it is about did run.  Frontier lengths are not compared between
forms: relax_packed reads its source's label live, so which round improves a vertex depends on timing.
"""
import functools
import itertools
import os
import re

import numpy as np
import pytest

from sssp_families import FAMILIES, FLT_MAX, INEXACT, inexact_share, overflow_graph, weights

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

INF_I = 2**31 - 1
FORM = re.compile(r"\[grx\] sssp iteration (\d+): form (\w) scan (\d) snapshot (\d) slots \d+ work (-?\d+)")
FORCED = {"GRX_SETTLED_MIN_WORK": "1", "GRX_FUSED_MIN_SLOTS": "64"}
PER_CALL = ("GRX_SSSP_PACKED", "GRX_SSSP_BOUND_FROM", "GRX_SSSP_EARLY_LIVE", "GRX_BFS_BYTE_LABELS")


@pytest.fixture
def gpu(oracle, monkeypatch):
    import torch
    import essentials_amd as ea
    assert torch.cuda.is_available()
    monkeypatch.setenv("GRX_DEBUG", "1")   # read once per run by the enactor
    for name in PER_CALL + tuple(FORCED) + ("GRX_LABEL_SCAN_MIN_WORK", "GRX_HOT_FIRST"):
        monkeypatch.delenv(name, raising=False)
    return ea


@functools.lru_cache(maxsize=1)
def rmat(oracle, scale, symmetric):
    """Generated once for the parametrised cases that share it (generation is most of their time)."""
    n, Ap, Aj, _ = oracle.rmat_csr(scale, 16, 1, 7, symmetric)
    return n, Ap, np.ascontiguousarray(Aj)


def per_call(monkeypatch, **env):
    """The knobs grx_sssp / grx_bfs read at every call: set the given ones, unset the others."""
    for name in PER_CALL:
        if env.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(env[name]))


def sssp(ea, ctx, G, s, capfd, options=None):
    """-> (distances on the host, Stats, [(form, scan, snapshot, work hint or -1) per iteration])."""
    capfd.readouterr()
    d, st = ea.sssp(ctx, G, int(s), options=options)
    got = d.cpu().numpy()
    lines = [m.groups() for m in FORM.finditer(capfd.readouterr().err)]
    assert [int(l[0]) for l in lines] == list(range(len(lines))) and lines, lines
    return got, st, [(l[1], int(l[2]), int(l[3]), int(l[4])) for l in lines]


def check(tag, got, st, want, deg):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (tag, f"{bad.size} of {len(want)} distances differ", bad[:5].tolist(),
                           got[bad[:5]].tolist(), want[bad[:5]].tolist())
    reached = want != FLT_MAX
    assert st.vertices_reached == int(reached.sum()), tag
    assert st.edges_traversed == int(deg[reached].sum()), tag
    assert st.edges_expanded >= st.edges_traversed, tag


def letters(forms):
    return "".join(f[0] for f in forms)


def bounded(forms):
    return [f for f in forms if f[0] in "CD"]


def scanned(forms):
    return [f for f in forms if f[1]]


def pick_sources(deg, rng):
    """0, the heaviest vertex (the heaviest other one where that is 0) and three seeded random ones
    with edges."""
    heaviest = int(np.argmax(deg[1:])) + 1
    others = np.flatnonzero(deg > 0)
    others = others[(others != 0) & (others != heaviest)]
    return [0, heaviest] + rng.choice(others, 3, replace=False).tolist()


def oracle_sssp(oracle, family, Ap, Aj, Ax, s):
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, int(s))
    if family in INEXACT:   # a condition on the input: the bound of nearly every distance is inexact
        assert inexact_share(want, int(s)) >= 0.99, (family, s)
    return want


@pytest.mark.parametrize("family", FAMILIES)
def test_default_thresholds_symmetric_rmat18(gpu, oracle, capfd, monkeypatch, family):
    """Default thresholds reach the bounded and the scan forms on RMAT-18 (8 M edges); every other
    formulation must arrive at the same bits."""
    ea = gpu
    ctx = ea.Context(0)
    n, Ap, Aj = rmat(oracle, 18, True)
    Ax = weights(family, Ap, Aj, 18, True)
    deg = np.diff(Ap)
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    sources = pick_sources(deg, np.random.default_rng(1800))
    want = {s: oracle_sssp(oracle, family, Ap, Aj, Ax, s) for s in sources}
    LB = ea.LoadBalance
    for hot in (True, False):
        if not hot:
            G.hot_first(ctx, False)
        seen = []
        for s in sources:
            per_call(monkeypatch)
            got, st, forms = sssp(ea, ctx, G, s, capfd)
            check((family, hot, s, letters(forms)), got, st, want[s], deg)
            assert ("E" in letters(forms)) <= hot      # early-live only on the hot-first copy
            seen += forms
            if not hot:
                continue
            per_call(monkeypatch, GRX_SSSP_PACKED=0)
            got, st, forms = sssp(ea, ctx, G, s, capfd)
            check((family, "two words", s), got, st, want[s], deg)
            assert set(letters(forms)) == {"W"}
            per_call(monkeypatch)
            for o, only in ((ea.Options(sssp_two_pass=True), "T"),
                            (ea.Options(load_balance=LB.merge_path), "A"),
                            (ea.Options(load_balance=LB.bucketing), "A")):
                got, st, forms = sssp(ea, ctx, G, s, capfd, o)
                check((family, o, s), got, st, want[s], deg)
                assert set(letters(forms)) == {only}, (o, letters(forms))
        print(f"[sssp wide] rmat18 {family} hot_first={hot}: "
              + " ".join(sorted({f"{a}{b}{c}" for a, b, c, _ in seen})))
        assert bounded(seen) and scanned(seen), (family, hot, seen)
    G.close()


@pytest.mark.parametrize("scale", [17, 20])
def test_default_thresholds_directed_with_sinks(gpu, oracle, capfd, monkeypatch, scale):
    """Directed R-MAT without attached in-edges: the hot-first copy is built, leading_connected counts
    the vertices with OUT-edges, and the sinks (in-edges only) lie beyond it.  Both label scans stop at
    leading_connected; the sinks are destinations all the same and must get the oracle's labels.

    RMAT-20 reaches every form with the default thresholds.  RMAT-17 (2 M edges) does not (witnessed):
    with `frac` its widest iterations expand 1.2 - 2.0 M edges, bounded (>= 2^20) but short of the scan
    threshold of 2^21 (forms A, E, C only); with `near` the one iteration after the early-live one
    expands 0.63 M edges, below 2^20, and no bounded iteration runs at all.  For that graph both
    thresholds are therefore forced down to 2^19."""
    ea = gpu
    if scale == 17:
        monkeypatch.setenv("GRX_SETTLED_MIN_WORK", str(1 << 19))
        monkeypatch.setenv("GRX_LABEL_SCAN_MIN_WORK", str(1 << 19))
    ctx = ea.Context(0)
    n, Ap, Aj = rmat(oracle, scale, False)
    deg = np.diff(Ap)
    indeg = np.bincount(Aj, minlength=n)
    sinks = (deg == 0) & (indeg > 0)
    assert sinks.sum() > 1000
    assert n >= (1 << 16) and len(Aj) >= (1 << 20)          # the copy is built without being asked for
    if scale == 20:
        assert int((deg > 0).sum()) < 786432 <= n           # settled_max_ids: the bitmap covers sinks
    sources = pick_sources(deg, np.random.default_rng(100 + scale))
    for family in ("frac", "near"):
        Ax = weights(family, Ap, Aj, scale, False)
        G = ea.Graph.from_host_csr(Ap, Aj, Ax)
        seen = []
        for s in sources:
            want = oracle_sssp(oracle, family, Ap, Aj, Ax, s)
            per_call(monkeypatch)
            got, st, forms = sssp(ea, ctx, G, s, capfd)
            check((scale, family, s, letters(forms)), got, st, want, deg)
            assert (got[sinks].view(np.uint32) == want[sinks].view(np.uint32)).all()
            assert (want[sinks] != FLT_MAX).sum() > 1000 or s != sources[1]
            seen += forms
        print(f"[sssp wide] directed rmat{scale} {family}: "
              + " ".join(sorted({f"{a}{b}{c}" for a, b, c, _ in seen})))
        assert bounded(seen) and scanned(seen), (scale, family, seen)
        G.close()
    G = ea.Graph.from_host_csr(Ap, Aj, np.ones(len(Aj), np.float32))
    for s in sources:
        want, _ = oracle.bfs_heap(Ap, Aj, int(s))
        for env, o in (({}, ea.Options()), ({"GRX_BFS_BYTE_LABELS": 1}, ea.Options()),
                       ({}, ea.Options(call_every_edge=True))):
            per_call(monkeypatch, **env)
            d, st = ea.bfs(ctx, G, int(s), options=o)
            d = d.cpu().numpy()
            assert (d == want).all(), (scale, s, env, o)
            assert (d[sinks] == want[sinks]).all()
            assert st.vertices_reached == int((want != INF_I).sum())
            assert st.edges_traversed == int(deg[want != INF_I].sum())
    G.close()


def forced_contexts(ea, monkeypatch):
    """The thresholds are read when a context is made: one context per value of the scan threshold,
    both with every iteration that has a work hint wide enough for the bounded form."""
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GRX_LABEL_SCAN_MIN_WORK", "1")
    with_scan = ea.Context(0)
    monkeypatch.delenv("GRX_LABEL_SCAN_MIN_WORK")
    without = ea.Context(0)
    return {True: with_scan, False: without}


def random_directed(rng, n):
    """Random directed graph with heavy destinations (as the BFS soak's), plus vertices without
    out-edges: sinks, and isolated ones that are no destination either."""
    m = int(rng.integers(0, 12 * n + 1))
    rows = np.sort(rng.integers(0, n, m)).astype(np.int32)
    hubs = rng.random(m) < 0.3
    cols = np.where(hubs, rng.integers(0, max(1, n // 50), m), rng.integers(0, n, m)).astype(np.int32)
    no_out = rng.random(n) < 0.15
    isolated = no_out & (rng.random(n) < 0.5)
    keep = ~no_out[rows] & ~isolated[cols]
    rows, cols = rows[keep], cols[keep]
    Ap = np.zeros(n + 1, np.int32)
    np.add.at(Ap, rows + 1, 1)
    return np.cumsum(Ap).astype(np.int32), np.ascontiguousarray(cols)


SIZES = [1, 2, 7, 63, 65, 129, 1000, 4097, 20011, 49151, 49152, 49153, 49160, 60001, 131071]


def test_forced_forms_on_small_and_odd_graphs(gpu, oracle, capfd, monkeypatch):
    """SSSP counterpart of test_settled_form_on_small_and_odd_graphs: every iteration with a work hint
    is wide (GRX_SETTLED_MIN_WORK=1), on sizes around the 49152 ids of the LDS bound image and sizes
    that are no multiple of 8, with every combination of the scan threshold, GRX_SSSP_BOUND_FROM,
    GRX_SSSP_EARLY_LIVE and hot-first numbering.  Iteration 0 (the source alone) carries no work hint
    and is always form A."""
    ea = gpu
    ctxs = forced_contexts(ea, monkeypatch)
    rng = np.random.default_rng(4242 + int(os.environ.get("GRX_STRESS_SEED", "0")))
    trials = int(os.environ.get("GRX_STRESS_TRIALS", "40"))
    combos = list(itertools.product((True, False), (None, 0, 2), (None, 0), (True, False)))
    seen = set()
    for trial in range(trials):
        scan, bound_from, early, hot = combos[trial % len(combos)]
        family = FAMILIES[(trial + trial // len(combos)) % len(FAMILIES)]
        n = SIZES[(trial * 7 + trial // len(SIZES)) % len(SIZES)] if trial < 2 * len(SIZES) else int(rng.choice(SIZES))
        Ap, Aj = random_directed(rng, n)
        Ax = weights(family, Ap, Aj, trial, False)
        deg = np.diff(Ap)
        G = ea.Graph.from_host_csr(Ap, Aj, Ax)
        G.hot_first(ctxs[scan], hot)
        for s in sorted({0, int(rng.integers(0, n)), int(np.argmax(deg))}):
            want, _ = oracle.sssp_heap(Ap, Aj, Ax, s)
            o = dict(hub_threshold=int(rng.choice([0, 4, 64])), chunk_edges=int(rng.choice([0, 8, 256])),
                     chunk_queue_limit=int(rng.choice([0, 0, 3])))
            per_call(monkeypatch, GRX_SSSP_BOUND_FROM=bound_from, GRX_SSSP_EARLY_LIVE=early)
            got, st, forms = sssp(ea, ctxs[scan], G, s, capfd, ea.Options(**o))
            tag = (trial, family, n, len(Aj), s, scan, bound_from, early, hot, o, letters(forms))
            check(tag, got, st, want, deg)
            assert forms[0][0] == "A" and forms[0][3] == -1, tag
            hot_copy = hot and n >= 2 and len(Aj) > 0
            plain = "E" if hot_copy and early is None else "B" if scan else "A"
            for i, (form, scanned_it, _, work) in enumerate(forms[1:], 1):
                if work == 0:                   # a frontier of sinks: nothing to expand
                    assert form == "A", tag
                    continue
                assert scanned_it == int(scan), tag          # scan iff the threshold says so
                if bound_from is None:          # by edges expanded so far: either side of that point
                    assert form in (plain, "D" if scan else "C"), tag
                else:
                    assert form == (("D" if scan else "C") if i >= bound_from else plain), tag
            seen |= {f[:3] for f in forms}
        G.close()
    print("[sssp wide] forced forms seen: " + " ".join(sorted(f"{a}{b}{c}" for a, b, c in seen)))
    if trials >= len(combos):
        assert {f[0] for f in seen} == set("ABCDE"), seen
        assert ("E", 1, 1) in seen and ("E", 0, 1) in seen and ("D", 1, 0) in seen and ("C", 0, 1) in seen, seen


def layered_graph_with_late_sinks(depth):
    """0 -> layer 1 -> ... -> layer `depth` (80 vertices each, every vertex with out-edges), and 60
    sinks: the odd ones are reached from layer `depth` only, the even ones also from layer 1 by an edge
    so heavy that layer `depth` improves them.  Ten isolated vertices come last."""
    width, n_sinks = 80, 60
    first_sink = 1 + depth * width
    n = first_sink + n_sinks + 10
    rows, cols = [], []

    def layer(k):
        return range(1 + (k - 1) * width, 1 + k * width)
    for v in layer(1):
        rows.append(0); cols.append(v)
    for k in range(1, depth):
        for i, v in enumerate(layer(k)):
            for j in (0, 1, 5):
                rows.append(v); cols.append(layer(k + 1)[(i + j) % width])
    heavy = []
    for i, v in enumerate(layer(1)):
        rows.append(v); cols.append(first_sink + 2 * (i % (n_sinks // 2))); heavy.append(len(rows) - 1)
    for i, v in enumerate(layer(depth)):
        for j in (0, 1, 2):
            rows.append(v); cols.append(first_sink + (i + 17 * j) % n_sinks)
    order = np.lexsort((cols, rows))
    is_heavy = np.zeros(len(rows), bool)
    is_heavy[heavy] = True
    rows = np.array(rows, np.int32)[order]
    Ap = np.zeros(n + 1, np.int32)
    np.add.at(Ap, rows + 1, 1)
    Ap = np.cumsum(Ap).astype(np.int32)
    Aj = np.ascontiguousarray(np.array(cols, np.int32)[order])
    Ax = weights("frac", Ap, Aj, 5, False)
    Ax[is_heavy[order]] = np.float32(1000.25)
    return Ap, Aj, Ax, np.arange(first_sink, first_sink + n_sinks)


@pytest.mark.parametrize("bound_from", [2, 3])
def test_scan_before_the_first_bounded_iteration_on_sinks(gpu, oracle, capfd, monkeypatch, bound_from):
    """Label scans (form B) run before the first bounded iteration on a hot-first DIRECTED graph:
    GRX_SSSP_EARLY_LIVE=0, scan threshold 1, GRX_SSSP_BOUND_FROM=2 (A, B, D) and 3 (A, B, B, D;
    iteration 0 has no work hint, so it is A whatever the knobs say).  The scan refreshes the bounds of
    the ids below leading_connected only.  Sinks lie beyond it, and the D iteration is the one that
    reaches or improves them, so it reads bound16[sink].  Before the fix that came with this test the
    scan declared the bounds fresh, D skipped snapshot_bounds and read values nothing had written
    (witness: D scan 1 snapshot 0).  Now the bounds count as fresh only once a snapshot has covered
    every id: the first bounded iteration must snapshot, later ones may rely on the scan."""
    ea = gpu
    ctx = forced_contexts(ea, monkeypatch)[True]
    Ap, Aj, Ax, sinks = layered_graph_with_late_sinks(bound_from)
    deg = np.diff(Ap)
    assert (deg[sinks] == 0).all() and (np.bincount(Aj, minlength=len(deg))[sinks] > 0).all()
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    G.hot_first(ctx, True)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    assert (want[sinks] < 1000).all() and inexact_share(want, 0) >= 0.99
    per_call(monkeypatch, GRX_SSSP_BOUND_FROM=bound_from, GRX_SSSP_EARLY_LIVE=0)
    for repeat in range(3):   # a handle re-used: the second run must not inherit "complete" bounds
        got, st, forms = sssp(ea, ctx, G, 0, capfd)
        check((bound_from, repeat, forms), got, st, want, deg)
        assert letters(forms) == "A" + "B" * (bound_from - 1) + "D", forms
        assert forms[-1][:3] == ("D", 1, 1), forms
    G.close()


def test_overflowing_path_sums(gpu, oracle, capfd, monkeypatch):
    """Path sums beyond FLT_MAX: the reference client's test is `d < atomic::min(...)`, an infinite
    candidate never replaces FLT_MAX, and the bound of an unreached label (0xff80 << 16 = the bits of
    +inf) rejects it.  oracle.sssp_heap reads it the same way (tests/test_sssp_families.py); the
    expected labels are written out by hand in sssp_families.overflow_graph and asserted too."""
    ea = gpu
    Ap, Aj, Ax, by_hand = overflow_graph()
    deg = np.diff(Ap)
    want, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    assert (want.view(np.uint32) == by_hand.view(np.uint32)).all()
    G = ea.Graph.from_host_csr(Ap, Aj, Ax)
    got, st, forms = sssp(ea, ea.Context(0), G, 0, capfd)
    check(("default", forms), got, st, want, deg)
    ctxs = forced_contexts(ea, monkeypatch)
    seen = set()
    for scan, bound_from, hot in itertools.product((True, False), (None, 0), (True, False)):
        G.hot_first(ctxs[scan], hot)
        per_call(monkeypatch, GRX_SSSP_BOUND_FROM=bound_from)
        got, st, forms = sssp(ea, ctxs[scan], G, 0, capfd)
        check((scan, bound_from, hot, forms), got, st, want, deg)
        seen |= {f[0] for f in forms}
    assert seen == set("ABCDE"), seen
    G.close()


def test_one_handle_many_sources_alternating_forms(gpu, oracle, capfd, monkeypatch):
    """Several sources in a row on ONE graph handle and ONE context per threshold set, the knobs (and
    with them the forms) changing from run to run: bounds, round tags and remembered frontiers of an
    earlier run must not leak into the next."""
    ea = gpu
    ctxs = forced_contexts(ea, monkeypatch)
    rng = np.random.default_rng(77)
    n = 49153
    Ap, Aj = random_directed(rng, n)
    deg = np.diff(Ap)
    graphs = {f: (weights(f, Ap, Aj, 9, False),) for f in ("near", "frac")}
    graphs = {f: (Ax, ea.Graph.from_host_csr(Ap, Aj, Ax)) for f, (Ax,) in graphs.items()}
    for _, G in graphs.values():
        G.hot_first(ctxs[True], True)
    sources = [0, int(np.argmax(deg))] + rng.choice(np.flatnonzero(deg > 0), 4, replace=False).tolist()
    want = {(f, s): oracle_sssp(oracle, f, Ap, Aj, graphs[f][0], s) for f in graphs for s in sources}
    knobs = [(True, None, None), (False, 0, None), (True, 2, 0), (False, None, 0), (True, 0, None),
             (True, None, 0), (False, None, None)]
    seen = set()
    for k, (s, f) in enumerate(itertools.product(sources + sources[::-1], graphs)):
        scan, bound_from, early = knobs[k % len(knobs)]
        per_call(monkeypatch, GRX_SSSP_BOUND_FROM=bound_from, GRX_SSSP_EARLY_LIVE=early)
        got, st, forms = sssp(ea, ctxs[scan], graphs[f][1], s, capfd)
        check((k, f, s, scan, bound_from, early, letters(forms)), got, st, want[(f, s)], deg)
        seen |= {x[0] for x in forms}
    assert seen == set("ABCDE"), seen
    for _, G in graphs.values():
        G.close()
