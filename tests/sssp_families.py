"""Edge-weight families and small graphs for the SSSP tests whose point is the 2-byte bound of the
wide iterations (clients.hxx: bound16 = the top 16 of a distance's order-preserving bits, rounded up).

An integer weight below 256 has at most 8 significant bits, so every distance built from such weights
has zero low 16 bits and the bound is exact: its rounding never decides anything.  The families here
make it decide.  All weights are non-negative float32 without denormals, and a pure function of
(family, seed, edge): the same edge gets the same weight wherever the graph is rebuilt, and on a
symmetric graph (u, v) and (v, u) get the same weight.

  frac   uniform in [0.1, 10): the low 16 bits of every reached distance are non-zero
  wide   2^uniform(-20, 20): thousands of distinct top-16 values
  near   1 + k 2^-23, k in [0, 4096): a handful of distinct top-16 values, so nearly every bound test
         ties in the top 16 bits and the rounding decides it
  zeros  integers in [1, 64], a fifth of the edges 0.0: equal distances, zero-weight cycles
"""
import heapq

import numpy as np

FAMILIES = ("frac", "wide", "near", "zeros")
INEXACT = ("frac", "wide", "near")   # families whose distances must have non-zero low 16 bits
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _splitmix(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def edge_uniform(Ap, Aj, seed, symmetric, stream=0):
    """One float64 in [0, 1) per edge, a hash of (seed, stream, endpoints); unordered endpoints when
    `symmetric`."""
    n = len(Ap) - 1
    src = np.repeat(np.arange(n, dtype=np.uint64), np.diff(Ap))
    dst = np.asarray(Aj).astype(np.uint64)
    if symmetric:
        src, dst = np.minimum(src, dst), np.maximum(src, dst)
    with np.errstate(over="ignore"):
        key = src * np.uint64(n) + dst
        h = _splitmix(_splitmix(key) ^ _splitmix(np.uint64(seed * 1000003 + stream * 7919 + 1)))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def weights(family, Ap, Aj, seed, symmetric):
    u = edge_uniform(Ap, Aj, seed, symmetric)
    if family == "frac":
        w = np.minimum((0.1 + 9.9 * u).astype(np.float32), np.float32(9.999999))
    elif family == "wide":
        w = np.exp2(-20.0 + 40.0 * u).astype(np.float32)
    elif family == "near":
        w = (1.0 + np.floor(u * 4096) * 2.0 ** -23).astype(np.float32)   # exact in float32
    elif family == "zeros":
        w = (1 + np.floor(u * 64)).astype(np.float32)
        w[edge_uniform(Ap, Aj, seed, symmetric, stream=1) < 0.2] = 0.0
    else:
        raise ValueError(family)
    w = np.ascontiguousarray(w, np.float32)
    assert (w >= 0).all() and np.isfinite(w).all()
    assert (w[w > 0] >= np.finfo(np.float32).tiny).all()   # no denormals
    return w


def inexact_share(dist, source):
    """Share of the reached vertices other than the source whose distance has non-zero low 16 bits."""
    reached = dist != FLT_MAX
    reached[source] = False
    if not reached.any():
        return 1.0
    return float(((dist.view(np.uint32)[reached] & 0xFFFF) != 0).mean())


def overflow_graph():
    """A small deterministic graph with path sums beyond FLT_MAX.

    0 -> 1..64 (1e38 each) -> 65..128 (1e38: 2e38, finite) -> 129..192 (3e38: the sum is +inf).
    A candidate of +inf is not below FLT_MAX, the label of an unreached vertex, so 129..192 and what
    only they lead to (193..200, weight 1) stay at FLT_MAX, i.e. unreached.  201 is reached both
    through an overflowing edge and through a finite one (2e38 + 1e38 = 3e38)."""
    rows, cols, vals = [], [], []

    def edge(u, v, w):
        rows.append(u); cols.append(v); vals.append(w)
    for i in range(64):
        edge(0, 1 + i, 1e38)
        edge(1 + i, 65 + i, 1e38)
        edge(1 + i, 65 + (i + 1) % 64, 1e38)
        edge(65 + i, 129 + i, 3e38)
        edge(65 + i, 129 + (i + 7) % 64, 3.4e38)
        edge(65 + i, 201, 3e38 if i % 2 else 1e38)
        edge(129 + i, 193 + i % 8, 1.0)
    n = 202
    order = np.lexsort((cols, rows))
    rows = np.array(rows, np.int32)[order]
    Ap = np.zeros(n + 1, np.int32)
    np.add.at(Ap, rows + 1, 1)
    Ap = np.cumsum(Ap).astype(np.int32)
    want = np.full(n, FLT_MAX, np.float32)
    want[0] = 0
    want[1:65] = np.float32(1e38)
    want[65:129] = np.float32(1e38) + np.float32(1e38)
    want[201] = want[65] + np.float32(1e38)
    return (Ap, np.ascontiguousarray(np.array(cols, np.int32)[order]),
            np.ascontiguousarray(np.array(vals, np.float32)[order]), want)


def dijkstra64(Ap, Aj, Ax, source):
    """float64 Dijkstra (heapq, stale entries skipped) -> (distances, inf if unreached; edges on the
    shortest path found)."""
    n = len(Ap) - 1
    dist = np.full(n, np.inf)
    hops = np.zeros(n, np.int64)
    dist[source] = 0.0
    w = Ax.astype(np.float64)
    heap = [(0.0, source)]
    while heap:
        d, v = heapq.heappop(heap)
        if d > dist[v]:
            continue
        for e in range(Ap[v], Ap[v + 1]):
            nb, nd = Aj[e], d + w[e]
            if nd < dist[nb]:
                dist[nb], hops[nb] = nd, hops[v] + 1
                heapq.heappush(heap, (nd, nb))
    return dist, hops


def tight_hops32(Ap, Aj, Ax, dist, source):
    """Fewest edges on a path from the source along which the left-to-right float32 sum IS dist[v]
    at every vertex (edges with float32(dist[u] + w) == dist[v]); -1 where there is none."""
    n = len(Ap) - 1
    src = np.repeat(np.arange(n), np.diff(Ap))
    tight = (dist[src] != FLT_MAX) & ((dist[src] + Ax).astype(np.float32) == dist[Aj])
    hops = np.full(n, -1, np.int64)
    hops[source] = 0
    frontier = np.array([source])
    level = 0
    while len(frontier):
        level += 1
        mask = tight & np.isin(src, frontier)
        nxt = np.unique(Aj[mask])
        nxt = nxt[hops[nxt] < 0]
        hops[nxt] = level
        frontier = nxt
    return hops
