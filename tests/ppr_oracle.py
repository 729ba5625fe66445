"""Oracle of grx_ppr: the definition in include/essentials_amd.h followed literally in numpy float64,
one independent run per seed.  The checker, never the thing shipped."""
import numpy as np

BATCH = 64
ULP = 2.0 ** -24


def csr(n, edges, weights=None, symmetric=True):
    """CSR (int32 ap, aj, float32 aw) of `edges` ([m, 2] vertex pairs) as given: repeats and loops
    stay; `weights` per pair (default 1), the same in both directions when symmetric."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if weights is None else np.asarray(weights, np.float64)
    if symmetric and len(e):
        e = np.concatenate([e, e[:, ::-1]])
        w = np.concatenate([w, w])
    order = np.argsort(e[:, 0], kind="stable")
    e, w = e[order], w[order]
    ap = np.zeros(n + 1, np.int64)
    np.add.at(ap, e[:, 0] + 1, 1)
    return np.cumsum(ap).astype(np.int32), e[:, 1].astype(np.int32), w.astype(np.float32)


def transpose(ap, aj, aw):
    """The in-edge arrays (tp, tj, tw) of a CSR: sources grouped by destination, stable."""
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap))
    order = np.argsort(np.asarray(aj, np.int64), kind="stable")
    tp = np.zeros(n + 1, np.int64)
    np.add.at(tp, np.asarray(aj, np.int64) + 1, 1)
    return np.cumsum(tp).astype(np.int32), src[order].astype(np.int32), np.asarray(aw)[order]


SWEEP_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 200]


def sweep_ladder():
    """The edge conditions of the lane-group row sweep at one tiny shape: a directed multigraph of 37
    vertices (no multiple of the 16 rows a workgroup walks side by side) whose out-rows AND in-rows have
    every length of SWEEP_LENGTHS -- around the group of 16, around a segment of 64 (64 is short, 65 is
    two items with a one-entry tail, 200 ends in a partial item) and none.  Vertex v < 11 has
    SWEEP_LENGTHS[v] out-entries and SWEEP_LENGTHS[(v + 2) % 11] in-entries: vertex 10 (200 out) is the
    source of the searches, vertex 9 (129 out, none in) is unreached with a long out-row.  The other
    26 vertices have 3 of each.  Weights are integers in [1, 8].  -> (ap, aj, aw)"""
    rng = np.random.default_rng(29)
    out_degree = np.array(SWEEP_LENGTHS + [3] * 26)
    in_degree = np.array([SWEEP_LENGTHS[(v + 2) % 11] for v in range(11)] + [3] * 26)
    tails = np.repeat(np.arange(37), out_degree)
    heads = rng.permutation(np.repeat(np.arange(37), in_degree))
    return csr(37, np.stack([tails, heads], axis=1), rng.integers(1, 9, len(tails)), symmetric=False)


def _setup(ap, aj, aw, alpha, in_edges):
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    aw = np.asarray(aw, np.float32).astype(np.float64)
    n = len(ap) - 1
    rows = np.repeat(np.arange(n), np.diff(ap))
    W = np.bincount(rows, weights=aw, minlength=n)[:n] if n else np.zeros(0)
    alpha = float(np.float32(alpha))
    scale = np.where(W != 0, alpha / np.where(W != 0, W, 1.0), 0.0)
    if in_edges is None:  # a symmetric CSR: row v's entries are v's in-entries
        tp, tj, tw = ap, aj, aw
    else:
        tp, tj = np.asarray(in_edges[0], np.int64), np.asarray(in_edges[1], np.int64)
        tw = np.asarray(in_edges[2], np.float32).astype(np.float64)
    dst = np.repeat(np.arange(n), np.diff(tp))
    return n, alpha, scale, W == 0, dst, tj, tw


def _run(setup, seed, tol, max_iterations, watch=None):
    """One seed: (p, iterations, residual).  watch(terms, p) sees every iteration's terms and result."""
    n, alpha, scale, dangling, dst, tj, tw = setup
    p = np.zeros(n)
    p[seed] = 1.0
    t, diff = 0, 0.0
    while True:
        terms = (p * scale)[tj] * tw
        new = np.bincount(dst, weights=terms, minlength=n)[:n]
        new[seed] += (1.0 - alpha) + alpha * p[dangling].sum()
        diff = float(np.abs(new - p).max())
        p = new
        t += 1
        if watch is not None:
            watch(terms, p)
        if (tol > 0 and diff < tol) or (max_iterations and t >= max_iterations):
            return p, t, diff


def ppr(ap, aj, aw, seeds=None, alpha=0.85, tol=1e-6, max_iterations=0, in_edges=None):
    """-> dict: p [count, V] float64, iterations (int32) and residual (float64) per seed, and the batch
    figures grx_stats defines: levels (per batch of 64 the largest iteration count), total (their sum),
    active (of the first batch: the columns not yet frozen when iteration t + 1 begins, at most 64
    entries) and reached (the entries whose float32 value is > 0)."""
    assert tol > 0 or max_iterations > 0
    tol = float(np.float32(tol))
    setup = _setup(ap, aj, aw, alpha, in_edges)
    n = setup[0]
    seeds = np.arange(n) if seeds is None else np.atleast_1d(np.asarray(seeds, np.int64))
    count = len(seeds)
    p = np.zeros((count, n))
    iterations = np.zeros(count, np.int32)
    residual = np.zeros(count)
    done = {}
    for i, s in enumerate(seeds):
        if n == 0:
            break
        if int(s) not in done:
            done[int(s)] = _run(setup, int(s), tol, max_iterations)
        p[i], iterations[i], residual[i] = done[int(s)]
    levels = [int(iterations[f:f + BATCH].max()) for f in range(0, count, BATCH)] if n else []
    active = [int((iterations[:BATCH] > t).sum()) for t in range(min(levels[0], 64))] if levels else []
    return {"p": p, "iterations": iterations, "residual": residual, "levels": levels, "total": sum(levels),
            "active": active, "reached": int((p.astype(np.float32) > 0).sum())}


def exact_in_float32(ap, aj, aw, seeds=None, alpha=0.85, tol=1e-6, max_iterations=0, in_edges=None):
    """True iff, at every iteration of the same run, every term p[u] * scale[u] * w and every value of
    p is an integer multiple of 2**-24 (and scale itself is a float32).  Non-negative multiples of
    2**-24 whose sums stay <= 1 add exactly in float32 in any order, so on such inputs a float32 run
    must match the float64 oracle bit for bit."""
    setup = _setup(ap, aj, aw, alpha, in_edges)
    n, scale = setup[0], setup[2]
    if not (scale.astype(np.float32).astype(np.float64) == scale).all():
        return False
    seeds = np.arange(n) if seeds is None else np.atleast_1d(np.asarray(seeds, np.int64))
    ok = [True]

    def watch(terms, p):
        for x in (terms, p):
            q = x / ULP
            if not ((q == np.round(q)).all() and (x >= 0).all() and (x <= 1).all()):
                ok[0] = False

    for s in set(int(s) for s in seeds):
        _run(setup, s, float(np.float32(tol)), max_iterations, watch)
    return ok[0]


def rounding_bound(max_in_row, n_dangling, alpha):
    """Bounds the L1 distance per column between a float32 run and the float64 run with the SAME
    iteration count.  Per iteration the rounding of a row sum of m terms is at most gamma(m + 2) times
    the row's true sum (m - 1 additions, the product and the scaling), the seed term adds
    gamma(n_dangling + 3), gamma(k) ~ k * 2**-24, a column's true sums add up to 1, and the operator
    contracts L1 by alpha, so the per-iteration errors sum to at most 1 / (1 - alpha) of one of them.
    The bound is derived, not measured."""
    return 1.01 * (max_in_row + n_dangling + 16) * ULP / (1.0 - alpha)


def exact_cases():
    """The inputs on which float32 is exact (checked by exact_in_float32 in tests/test_ppr_abi.py):
    name -> dict(ap, aj, aw, directed, seeds, alpha, tol, T).  T == 0: the run stops by tol."""
    cases = {}

    def add(name, n, edges, seeds, T, weights=None, directed=False, tol=0.0):
        ap, aj, aw = csr(n, edges, weights, symmetric=not directed)
        cases[name] = dict(ap=ap, aj=aj, aw=aw, directed=directed, seeds=seeds, alpha=0.5, tol=tol, T=T)

    ring = [(v, (v + 1) % 8) for v in range(8)]
    add("ring", 8, ring, [0], 12)
    add("cube", 16, [(v, v ^ (1 << b)) for v in range(16) for b in range(4) if v < v ^ (1 << b)], [0, 5], 8)
    add("star", 4097, [(0, v) for v in range(1, 4097)], [0, 7], 3)
    add("path", 6, [(v, v + 1) for v in range(5)], [0, 3, 5], 12, directed=True)
    k4 = [(u, (u + d) % 4) for u in range(4) for d in (1, 2, 3)]
    add("k4", 4, k4, [0, 2], 8, weights=[2.0 if d == 1 else 1.0 for u in range(4) for d in (1, 2, 3)], directed=True)
    add("ring_isolated", 9, ring, [0, 8], 0, tol=2.0 ** -8)
    return cases
