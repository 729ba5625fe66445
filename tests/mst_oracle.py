"""Minimum spanning forest of a CSR as grx_mst defines it, in plain numpy (the GPU machine may lack
scipy and networkx).  Every row entry e = (u, v, w) -- e its position in the column array -- is an
undirected candidate; entries are strictly ordered by key(e) = (ordered_bits(w) << 32) | e, and the
answer is the set of entries Kruskal accepts in ascending key.

forest()   a vectorised Boruvka on those keys: per round np.minimum.at of the live keys into both
           ends' components, every component with a key hooks under the one at the other end (of two
           that picked the same entry the smaller id stays), pointer jumping, the dead entries
           dropped.  The strict order makes the result Kruskal's whatever the rounds look like.
kruskal()  the definition itself: a Python sort and a union-find.  For small graphs.

Both return (sorted int32 entries, float64 weight, int32 labels); the labels are those of
cc_oracle.components (the smallest vertex id of each component).  The weight is numpy's float64 sum
of the chosen float32 values in ascending entry order; grx_mst adds them in another fixed tree, so
the two agree bit for bit whenever that sum is exact (small integers and dyadic fractions: every
graph of the tests)."""
import numpy as np

from tc_oracle import csr, mtx_csr  # noqa: F401  (re-exported for the tests)

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def ordered_bits(ax):
    """Monotone float32 -> uint32: the bits inverted under a set sign, the sign set otherwise."""
    b = np.ascontiguousarray(ax, np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def keys(ax):
    return (ordered_bits(ax).astype(np.uint64) << np.uint64(32)) | np.arange(len(ax), dtype=np.uint64)


def _ends(ap, aj):
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    return n, src, np.asarray(aj, np.int64)[: len(src)]


def _result(n, comp, chosen, ax):
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    entries = np.flatnonzero(chosen).astype(np.int32)
    weight = float(np.asarray(ax, np.float32)[entries].astype(np.float64).sum())
    return entries, weight, smallest[comp].astype(np.int32)


def forest(ap, aj, ax):
    n, src, dst = _ends(ap, aj)
    key = keys(np.asarray(ax, np.float32)[: len(src)])
    comp = np.arange(n, dtype=np.int64)
    chosen = np.zeros(len(src), bool)
    rounds = 0
    while True:
        cs, cd = comp[src], comp[dst]
        live = cs != cd
        if not live.any():
            break
        src, dst, key, cs, cd = src[live], dst[live], key[live], cs[live], cd[live]
        best = np.full(n, NONE, np.uint64)
        np.minimum.at(best, cs, key)
        np.minimum.at(best, cd, key)
        roots = np.flatnonzero(best != NONE)
        e = (best[roots] & np.uint64(0xFFFFFFFF)).astype(np.int64)  # positions in the whole CSR
        at = np.searchsorted(key & np.uint64(0xFFFFFFFF), e.astype(np.uint64))  # ... in the live arrays
        other = np.where(cs[at] == roots, cd[at], cs[at])
        stays = (best[other] == best[roots]) & (roots < other)  # both picked this entry
        link = np.arange(n, dtype=np.int64)
        link[roots[~stays]] = other[~stays]
        chosen[e[~stays]] = True
        while True:
            nxt = link[link]
            if (nxt == link).all():
                break
            link = nxt
        comp = link[comp]
        rounds += 1
        assert rounds <= max(n, 2).bit_length() + 1
    return _result(n, comp, chosen, ax)


def kruskal(ap, aj, ax):
    n, src, dst = _ends(ap, aj)
    key = keys(np.asarray(ax, np.float32)[: len(src)])
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    chosen = np.zeros(len(src), bool)
    for e in np.argsort(key, kind="stable").tolist():
        a, b = find(int(src[e])), find(int(dst[e]))
        if a != b:
            parent[a] = b
            chosen[e] = True
    comp = np.array([find(v) for v in range(n)], np.int64)
    return _result(n, comp, chosen, ax)


def weighted_csr(n, edges, weights, symmetric=True):
    """Row-sorted CSR (int32, int32, float32) of a weighted edge list; both directions when
    `symmetric`, a self loop then twice, repeats kept."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(weights, np.float32).reshape(-1)
    if symmetric:
        e, w = np.concatenate([e, e[:, ::-1]]), np.concatenate([w, w])
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, w = e[order], w[order]
    ap = np.zeros(n + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(e[:, 0], minlength=n))
    return ap.astype(np.int32), e[:, 1].astype(np.int32), w


def _k3(first, at):
    """Rows of a triangle on first .. first + 2, every weight 1; `at` is its first position."""
    a, b, c = first, first + 1, first + 2
    return [[(b, 1), (c, 1)], [(a, 1), (c, 1)], [(a, 1), (b, 1)]], [at, at + 1]


def _known():
    k = {}
    k["empty"] = ([], [], 0.0)
    k["isolated"] = ([[] for _ in range(5)], [], 0.0)
    k["only_a_self_loop"] = ([[], [(1, 2.0)], []], [], 0.0)
    # 0-1 (3), 1-2 (1), 0-2 (2): positions 0 1 | 2 3 | 4 5
    k["triangle_distinct"] = ([[(1, 3), (2, 2)], [(0, 3), (2, 1)], [(0, 2), (1, 1)]], [1, 3], 3.0)
    # every weight equal: the lowest positions win
    k["triangle_equal"] = (_k3(0, 0)[0], [0, 1], 2.0)
    # square 0-1 (1), 1-2 (2), 2-3 (3), 3-0 (4) and the diagonal 0-2 (2.5): 0 1 2 | 3 4 | 5 6 7 | 8 9
    k["square_and_diagonal"] = ([[(1, 1), (2, 2.5), (3, 4)], [(0, 1), (2, 2)], [(0, 2.5), (1, 2), (3, 3)],
                                 [(0, 4), (2, 3)]], [0, 4, 7], 6.0)
    k["two_cliques"] = (_k3(0, 0)[0] + _k3(3, 6)[0], [0, 1, 6, 7], 4.0)
    # the bridge 2-3 (5): 0 1 | 2 3 | 4 5 6 | 7 8 9 | 10 11 | 12 13
    k["two_cliques_bridge"] = ([[(1, 1), (2, 1)], [(0, 1), (2, 1)], [(0, 1), (1, 1), (3, 5)],
                                [(2, 5), (4, 1), (5, 1)], [(3, 1), (5, 1)], [(3, 1), (4, 1)]], [0, 1, 6, 8, 9], 9.0)
    k["repeated_edge_lighter_wins"] = ([[(1, 5), (1, 2)], [(0, 5), (0, 2)]], [1], 2.0)
    k["repeated_edge_earlier_wins"] = ([[(1, 2), (1, 2)], [(0, 2), (0, 2)]], [0], 2.0)
    k["directed_chain"] = ([[(1, 4)], [(2, 3)], [(3, 2)], [(4, 1)], []], [0, 1, 2, 3], 10.0)
    k["directed_in_star"] = ([[(2, 1)], [(2, 2)], [], [(2, 4)], [(2, 5)]], [0, 1, 2, 3], 12.0)
    k["minus_zero_before_plus_zero"] = ([[(1, 0.0), (1, -0.0)], []], [1], 0.0)
    # 0-1 (-1), 1-2 (-3), 0-2 (2)
    k["negative_weights"] = ([[(1, -1), (2, 2)], [(0, -1), (2, -3)], [(0, 2), (1, -3)]], [0, 3], -4.0)
    return k


# name -> (rows: for each vertex its list of (neighbour, weight), chosen positions, total weight)
KNOWN = _known()


def known_csr(name):
    rows, entries, weight = KNOWN[name]
    ap = np.zeros(len(rows) + 1, np.int32)
    ap[1:] = np.cumsum([len(r) for r in rows])
    aj = np.array([v for r in rows for v, _ in r], np.int32)
    ax = np.array([w for r in rows for _, w in r], np.float32)
    return ap, aj, ax, np.asarray(entries, np.int32), float(weight)
