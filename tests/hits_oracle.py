"""Oracle of grx_hits and grx_spmv: the definitions in include/essentials_amd.h followed literally in
numpy float64.  The checker, never the thing shipped."""
import numpy as np

# the tests build their inputs with these
from ppr_oracle import SWEEP_LENGTHS, csr, sweep_ladder, transpose  # noqa: F401

ULP = 2.0 ** -24


def _rows(ap, aj, aw):
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    aw = np.asarray(aw, np.float32).astype(np.float64)
    return np.repeat(np.arange(len(ap) - 1), np.diff(ap)), aj, aw


def spmv(ap, aj, aw, x, n_cols=None, transpose=False):
    """y = A x (float64), or y = A^T x: y[c] = sum over entries (r -> c, w) of x[r] * w."""
    row, col, w = _rows(ap, aj, aw)
    n = len(ap) - 1
    x = np.asarray(x, np.float64)
    if transpose:
        m = n if n_cols is None else n_cols
        return np.bincount(col, weights=x[row] * w, minlength=m)[:m] if m else np.zeros(0)
    return np.bincount(row, weights=x[col] * w, minlength=n)[:n] if n else np.zeros(0)


def _scaled(v):
    m = float(np.abs(v).max()) if len(v) else 0.0
    return v / m if m != 0 else np.zeros_like(v)


def _run(ap, aj, aw, tol, max_iterations, in_edges, watch=None):
    src, dst, w = _rows(ap, aj, aw)           # out-entries (src -> dst, w)
    n = len(ap) - 1
    if in_edges is None:                      # a symmetric CSR: row v's entries are v's in-entries
        head, tail, tw = src, dst, w          # in-entries (tail -> head, tw)
    else:
        head, tail, tw = _rows(*in_edges)
    h = np.ones(n)
    a = np.zeros(n)
    history = []
    t = 0
    while n:
        t_in = h[tail] * tw
        a = _scaled(np.bincount(head, weights=t_in, minlength=n)[:n])
        t_out = a[dst] * w
        new = _scaled(np.bincount(src, weights=t_out, minlength=n)[:n])
        history.append(float(np.abs(new - h).max()))
        h = new
        t += 1
        if watch is not None:
            watch((head, t_in), (src, t_out), a, h)
        if (tol > 0 and history[-1] < tol) or (max_iterations and t >= max_iterations):
            break
    return a, h, t, history


def hits(ap, aj, aw, tol, max_iterations=0, in_edges=None):
    """-> dict: a and h (float64, largest magnitude 1 or all 0), iterations, residuals (one per
    iteration; the last is what the call reports), and the stats the answer defines: edges
    (2 * nnz * iterations) and reached (the vertices whose float32 hub or authority value is > 0)."""
    assert tol > 0 or max_iterations > 0
    a, h, t, history = _run(ap, aj, aw, float(np.float32(tol)), max_iterations, in_edges)
    reached = int(((a.astype(np.float32) > 0) | (h.astype(np.float32) > 0)).sum())
    return {"a": a, "h": h, "iterations": t, "residuals": history, "residual": history[-1] if history else 0.0,
            "edges": 2 * len(np.asarray(aj)) * t, "reached": reached}


def _low_bit(values):
    """The largest power of two that divides each (positive, finite) value; inf for 0."""
    mantissa, exponent = np.frexp(values)            # value = mantissa * 2**exponent, mantissa in [0.5, 1)
    scaled = np.round(mantissa * 2.0 ** 53).astype(np.int64)
    low = (scaled & -scaled).astype(np.float64)      # lowest set bit of the 53-bit mantissa
    return np.where(values > 0, low * 2.0 ** (exponent.astype(np.float64) - 53), np.inf)


def exact_in_float32(ap, aj, aw, tol, max_iterations=0, in_edges=None):
    """True iff at every iteration of the same run every term and every vector entry is non-negative
    and, sum by sum, the terms of a row are integer multiples of one quantum q = 2**k with the row
    total below 2**24 * q.  Then every partial sum of the row, in any order, is a multiple of q below
    2**24 * q: a float32 holds it, no addition rounds (a fused multiply-add rounds once, to the same
    value), and any summation order gives the float64 result bit for bit.  The scaling must be exact
    however it is carried out, so every maximum has to be a power of two: dividing by it and
    multiplying by its reciprocal then both only change the exponent."""
    ok = [True]

    def watch(in_terms, out_terms, a, h):
        n = len(a)
        for (owner, terms), scaled in ((in_terms, a), (out_terms, h)):
            if not (np.isfinite(terms).all() and (terms >= 0).all() and (scaled >= 0).all()):
                ok[0] = False
                return
            quantum = np.full(n, np.inf)
            np.minimum.at(quantum, owner, _low_bit(terms))
            totals = np.bincount(owner, weights=terms, minlength=n)[:n]
            if not (totals[totals > 0] < 2.0 ** 24 * quantum[totals > 0]).all():
                ok[0] = False
            largest = totals.max() if n else 0.0
            if largest > 0 and np.frexp(largest)[0] != 0.5:
                ok[0] = False
            if not (scaled.astype(np.float32).astype(np.float64) == scaled).all():
                ok[0] = False

    _run(ap, aj, aw, float(np.float32(tol)), max_iterations, in_edges, watch)
    return ok[0]


def rounding_bound(T, D):
    """Bounds max_v |float32 run - float64 run| after T iterations, for both vectors, at equal
    iteration count and non-negative weights; D is the longest row or in-row.  With u = 2**-24 and
    gamma(k) ~ k * u:

    Every computed vector is c * (1 + e_v) * (the exact unnormalised vector)_v for one scalar c > 0
    and a componentwise relative error e: the maximum is a scalar, and non-negative terms cannot
    cancel, so a relative error of the operand becomes at most the same relative error of the sum.
    One product adds to the bound on |e|: gamma(D + 1) for a row sum of at most D terms in any order
    (D - 1 additions and the products, fused or not), and two roundings for the scaling (the
    reciprocal of the maximum, then the multiplication; a division is one).  That is (D + 3) u per
    product, and there are 2 T products: |e| <= 2 T (D + 3) u for either vector.
    The delivered vector is x_v / max(x): the maximum carries the same relative error, so the
    quotient's error is at most doubled, 4 T (D + 3) u, times an exact value that is at most 1; the
    final rounding of an entry at most 1 adds u.  The factor 1.01 covers the second-order terms.
    The bound is derived, not measured."""
    return 1.01 * (4 * T * (D + 3) + 1) * ULP


def exact_cases():
    """The inputs on which float32 is exact (checked by exact_in_float32 in tests/test_hits_abi.py):
    name -> dict(ap, aj, aw, directed, tol, T).  T == 0: the run stops by tol."""
    cases = {}

    def add(name, n, edges, tol=0.0, T=0, weights=None, directed=True):
        ap, aj, aw = csr(n, edges, weights, symmetric=not directed)
        cases[name] = dict(ap=ap, aj=aj, aw=aw, directed=directed, tol=tol, T=T)

    add("ring", 8, [(v, (v + 1) % 8) for v in range(8)], tol=2.0 ** -8, directed=False)
    add("two_edges", 4, [(0, 1), (2, 3)], tol=2.0 ** -8, weights=[2.0, 1.0])
    add("k24_plus_edge", 8, [(u, v) for u in (0, 1) for v in (2, 3, 4, 5)] + [(6, 7)], tol=2.0 ** -10)
    add("out_star", 4097, [(0, v) for v in range(1, 4097)], tol=2.0 ** -8)
    add("in_star", 4097, [(v, 0) for v in range(1, 4097)], tol=2.0 ** -8)
    add("path_w", 4, [(0, 1), (1, 2), (2, 3)], T=6, weights=[4.0, 2.0, 1.0])
    return cases


def case_in_edges(c):
    return transpose(c["ap"], c["aj"], c["aw"]) if c["directed"] else None
