"""CPU checks of what tests/test_gpu_sssp_wide.py relies on: the float32 oracle against a float64
Dijkstra on every weight family, the families' own properties, and the oracle's reading of path sums
beyond FLT_MAX."""
import numpy as np
import pytest

from sssp_families import (FAMILIES, FLT_MAX, INEXACT, dijkstra64, inexact_share, overflow_graph,
                           tight_hops32, weights)


@pytest.mark.parametrize("family", FAMILIES)
def test_float32_oracle_against_float64_dijkstra(oracle, family):
    """oracle.sssp_heap sums in float32, left to right along a path.  A sum of h terms starting from
    0 rounds h - 1 times, each by at most 2^-24 relative, and all terms are non-negative, so the
    float32 sum along any path is within h 2^-24 (relative) of its exact sum.  Upper side: the
    float32 fix point is at most the float32 sum along the float64 search's path.  Lower side: it IS
    the float32 sum along a path of tight edges, whose exact sum is at least the float64 distance.
    Hence |d32 - d64| <= max(h64, h32) 2^-24 d64 with the hop counts of those two paths."""
    n, Ap, Aj, _ = oracle.rmat_csr(10, 8, 5, 7, family != "wide")   # one directed graph among them
    Aj = np.ascontiguousarray(Aj)
    Ax = weights(family, Ap, Aj, 11, family != "wide")
    source = int(np.argmax(np.diff(Ap)))
    d32, _ = oracle.sssp_heap(Ap, Aj, Ax, source)
    d64, h64 = dijkstra64(Ap, Aj, Ax, source)
    reached = np.isfinite(d64)
    assert ((d32 != FLT_MAX) == reached).all()
    assert reached.sum() > n // 4
    h32 = tight_hops32(Ap, Aj, Ax, d32, source)
    assert (h32[reached] >= 0).all()
    hops = np.maximum(h64, h32)[reached]
    err = np.abs(d32[reached].astype(np.float64) - d64[reached])
    assert (err <= hops * 2.0 ** -24 * d64[reached]).all(), (family, float(err.max()))
    if family in INEXACT:
        assert inexact_share(d32, source) >= 0.99, family
    else:   # integer weights: exact sums, and zero-weight edges give equal distances
        assert (err == 0).all() and inexact_share(d32, source) == 0.0
        assert (Ax == 0).mean() > 0.15


def test_weights_are_a_function_of_the_edge(oracle):
    n, Ap, Aj, _ = oracle.rmat_csr(9, 8, 2, 7, True)
    Aj = np.ascontiguousarray(Aj)
    src = np.repeat(np.arange(n), np.diff(Ap))
    for family in FAMILIES:
        w = weights(family, Ap, Aj, 3, True)
        assert (w == weights(family, Ap, Aj, 3, True)).all()
        assert (w != weights(family, Ap, Aj, 4, True)).mean() > 0.5
        table = {}
        for u, v, x in zip(src.tolist(), Aj.tolist(), w.tolist()):
            assert table.setdefault((min(u, v), max(u, v)), x) == x


def test_oracle_on_path_sums_beyond_flt_max(oracle):
    """The reference client relaxes with `d < atomic::min(&distance[dst], d)`: a candidate of +inf is
    not below FLT_MAX, so a vertex only such sums lead to keeps FLT_MAX.  The oracle reads it the
    same way."""
    Ap, Aj, Ax, want = overflow_graph()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(2e38) + np.float32(3e38))
    got, _ = oracle.sssp_heap(Ap, Aj, Ax, 0)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got[129:201] == FLT_MAX).all() and got[201] < FLT_MAX
