"""Core numbers of a symmetric CSR by peeling on the entries as they are given, in plain numpy (the
GPU machine may lack scipy and networkx).  The degree of v is the length of row v: a repeated entry
counts each time, a self loop once.  Level by level (k = the smallest remaining degree, so empty
levels are skipped), round by round: the vertices of remaining degree <= k leave together, and
np.subtract.at lowers the degree of the vertex named by every entry of their rows."""
import numpy as np

from tc_oracle import csr, mtx_csr  # noqa: F401  (re-exported for the tests)


def core_numbers(ap, aj):
    """(int32 core numbers, degeneracy, levels = distinct non-zero core values)."""
    ap = np.asarray(ap, np.int64)
    aj = np.asarray(aj, np.int64)
    n = len(ap) - 1
    length = np.diff(ap)
    deg = length.copy()
    core = np.zeros(n, np.int32)
    inside = deg > 0
    left = int(inside.sum())
    k = levels = 0
    while left:
        k = int(deg[inside].min())
        levels += 1
        leaving = np.flatnonzero(inside & (deg <= k))
        while len(leaving):
            core[leaving] = k
            inside[leaving] = False
            left -= len(leaving)
            lens = length[leaving]
            first = np.cumsum(lens) - lens
            named = aj[np.repeat(ap[leaving] - first, lens) + np.arange(int(lens.sum()))]
            np.subtract.at(deg, named, 1)
            hit = named[inside[named] & (deg[named] <= k)]
            leaving = np.unique(hit)
    return core, k, levels


def simple_csr(ap, aj, ax=None):
    """The simple graph under a CSR: self loops dropped, repeated entries once (the smallest weight
    of the repeats), rows sorted by column.  (ap, aj) as int32, plus float32 weights when given."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    keep = row != col
    key, inverse = np.unique(row[keep] * max(n, 1) + col[keep], return_inverse=True)
    out_ap = np.zeros(n + 1, np.int64)
    out_ap[1:] = np.cumsum(np.bincount(key // max(n, 1), minlength=n))
    out = out_ap.astype(np.int32), (key % max(n, 1)).astype(np.int32)
    if ax is None:
        return out
    w = np.full(len(key), np.inf, np.float64)
    np.minimum.at(w, inverse.reshape(-1), np.asarray(ax, np.float64)[: len(row)][keep])
    return out + (w.astype(np.float32),)


def write_mtx(path, ap, aj):
    """Lower triangle of a symmetric CSR without self loops as 'coordinate pattern symmetric'."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    low = row > col
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate pattern symmetric\n")
        f.write(f"{n} {n} {int(low.sum())}\n")
        np.savetxt(f, np.stack([row[low] + 1, col[low] + 1], 1), fmt="%d %d")


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


def _known():
    k = {}
    for n in (2, 5, 12):
        k[f"complete{n}"] = (n, _clique(0, n), True, [n - 1] * n)
    k["cycle"] = (9, [(i, (i + 1) % 9) for i in range(9)], True, [2] * 9)
    k["path"] = (30, [(i, i + 1) for i in range(29)], True, [1] * 30)
    k["star"] = (30, [(0, i) for i in range(1, 30)], True, [1] * 30)
    k["isolated"] = (9, [], True, [0] * 9)
    k["empty"] = (0, [], True, [])
    k["k4_every_edge_three_times"] = (4, _clique(0, 4) * 3, True, [9] * 4)
    k["k5_pendant_path"] = (8, _clique(0, 5) + [(4, 5), (5, 6), (6, 7)], True, [4] * 5 + [1] * 3)
    k["two_cliques_bridge"] = (9, _clique(0, 4) + _clique(4, 5) + [(3, 4)], True, [3] * 4 + [4] * 5)
    k["only_a_self_loop"] = (3, [(0, 0)], False, [1, 0, 0])
    return k


# name -> (V, edge list, add both directions, core numbers)
KNOWN = _known()


def known_csr(name):
    n, edges, both, want = KNOWN[name]
    ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2), symmetric=both)
    return ap, aj, np.asarray(want, np.int32)
