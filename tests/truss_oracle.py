"""Trussness of every edge of the simple undirected graph under a symmetric CSR, by set-based
peeling in plain Python (the GPU machine may lack scipy and networkx).  The convention is that of
networkx.k_truss: truss(e) is the largest k >= 2 such that e lies in a subgraph whose every edge
closes at least k - 2 triangles inside it.  Level by level (k - 2 = the smallest remaining support
when nobody is at the floor, so empty levels are skipped), edge by edge: an edge at or below the
floor leaves, and every triangle it was in costs its two other edges one, never below the floor."""
import numpy as np

from kcore_oracle import csr, mtx_csr, simple_csr  # noqa: F401  (re-exported for the tests)


def truss_numbers(ap, aj):
    """(int32 trussness per CSR entry with self loops at 0, the largest value, levels = distinct
    values over the edges)."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap)).tolist()
    dst = np.asarray(aj, np.int64)[: len(src)].tolist()
    adj = [set() for _ in range(n)]
    for u, v in zip(src, dst):
        if u != v:
            adj[u].add(v)
            adj[v].add(u)
    support = {(u, v): len(adj[u] & adj[v]) for u in range(n) for v in adj[u] if u < v}
    truss = {}
    k, levels = 2, 0
    while support:
        floor = k - 2
        leaving = [e for e, s in support.items() if s <= floor]
        if not leaving:
            k = min(support.values()) + 2
            continue
        levels += 1
        while leaving:
            e = leaving.pop()
            u, v = e
            del support[e]
            truss[e] = k
            adj[u].discard(v)
            adj[v].discard(u)
            for w in adj[u] & adj[v]:
                for f in ((min(u, w), max(u, w)), (min(v, w), max(v, w))):
                    if support[f] > floor:
                        support[f] -= 1
                        if support[f] == floor:
                            leaving.append(f)
        k += 1
    per_entry = np.fromiter((0 if u == v else truss[(min(u, v), max(u, v))] for u, v in zip(src, dst)),
                            np.int32, len(src))
    return per_entry, max(truss.values(), default=0), levels


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


# name -> (V, undirected edge list, the trussness of each listed edge)
KNOWN = {
    "empty": (0, [], []),
    "isolated": (9, [], []),
    "one_edge": (2, [(0, 1)], [2]),
    "triangle": (3, [(0, 1), (1, 2), (0, 2)], [3, 3, 3]),
    "k4_minus_an_edge": (4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)], [3, 3, 3, 3, 3]),
    "two_triangles_sharing_an_edge": (5, [(1, 2), (2, 4), (1, 4), (2, 3), (3, 4)], [3, 3, 3, 3, 3]),
    "complete5": (5, _clique(0, 5), [5] * 10),
    "complete5_with_a_pendant_edge": (6, _clique(0, 5) + [(4, 5)], [5] * 10 + [2]),
    "complete12": (12, _clique(0, 12), [12] * 66),
}


def known_csr(name):
    """(ap, aj, the written-out answer per CSR entry) of a KNOWN graph."""
    n, edges, values = KNOWN[name]
    ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2))
    of = {}
    for (a, b), t in zip(edges, values):
        of[(a, b)] = of[(b, a)] = t
    src = np.repeat(np.arange(n), np.diff(ap)).tolist()
    want = np.asarray([of[(u, int(v))] for u, v in zip(src, aj)], np.int32)
    return ap, aj, want


def entry_values(ap, aj, values):
    """{(u, v): the set of values its entries carry} of a per-entry array."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap)).tolist()
    out = {}
    for u, v, t in zip(src, np.asarray(aj).tolist(), np.asarray(values).tolist()):
        out.setdefault((u, v), set()).add(t)
    return out
