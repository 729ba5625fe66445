"""Triangle counts of the simple undirected graph under a CSR, in plain numpy (the GPU machine may
lack scipy and networkx): repeated entries and self loops dropped, edges oriented by (degree, id),
every 2-path u -> v -> w closed by a searchsorted test of u -> w, counts gathered by np.add.at."""
import numpy as np


def simple_edges(ap, aj):
    """Distinct undirected edges (a < b) of the CSR, self loops dropped, as two int64 arrays."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    dst = np.asarray(aj, np.int64)[: len(src)]
    keep = src != dst
    a, b = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    key = np.unique(a * n + b)
    return key // max(n, 1), key % max(n, 1)


def simple_degrees(ap, aj):
    n = len(ap) - 1
    a, b = simple_edges(ap, aj)
    return np.bincount(a, minlength=n) + np.bincount(b, minlength=n)


def triangles(ap, aj, chunk=1 << 22):
    """(int64 per-vertex triangle counts, number of distinct triangles T)."""
    n = len(ap) - 1
    counts = np.zeros(n, np.int64)
    a, b = simple_edges(ap, aj)
    if not len(a):
        return counts, 0
    deg = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    # orient low (degree, id) -> high
    a_first = (deg[a] < deg[b]) | ((deg[a] == deg[b]) & (a < b))
    x, y = np.where(a_first, a, b), np.where(a_first, b, a)
    key = np.sort(x * n + y)
    x, y = key // n, key % n
    op = np.zeros(n + 1, np.int64)
    op[1:] = np.cumsum(np.bincount(x, minlength=n))
    outdeg = np.diff(op)
    total = 0
    # every oriented edge u -> v with out(v), in chunks of about `chunk` 2-paths
    work = np.cumsum(outdeg[y])
    lo = 0
    while lo < len(x):
        hi = int(np.searchsorted(work, (work[lo - 1] if lo else 0) + chunk, side="right"))
        hi = max(hi, lo + 1)
        u, v = x[lo:hi], y[lo:hi]
        lens = outdeg[v]
        m = int(lens.sum())
        lo = hi
        if not m:
            continue
        first = np.cumsum(lens) - lens
        pos = np.repeat(op[v] - first, lens) + np.arange(m)
        uu, vv, ww = np.repeat(u, lens), np.repeat(v, lens), y[pos]
        q = uu * n + ww
        at = np.searchsorted(key, q)
        hit = (at < len(key)) & (key[np.minimum(at, len(key) - 1)] == q)
        total += int(hit.sum())
        for side in (uu, vv, ww):
            np.add.at(counts, side[hit], 1)
    return counts, total


def csr(n, edges, symmetric=True):
    """Row-sorted CSR (int32) of an edge list; both directions when `symmetric`."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if symmetric:
        e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    ap = np.zeros(n + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(e[:, 0], minlength=n))
    return ap.astype(np.int32), e[:, 1].astype(np.int32)


def mtx_csr(path):
    """Row-sorted CSR of a 'coordinate pattern symmetric' Matrix Market file, both directions."""
    with open(path) as f:
        lines = [l for l in f if not l.startswith("%")]
    n = int(lines[0].split()[0])
    e = np.array([l.split()[:2] for l in lines[1:] if l.strip()], np.int64) - 1
    return csr(n, e)


# the two graphs of the reference's unit test (unittests/algorithms/tc.cuh): counts [2, 1, 2, 1]
KNOWN = {
    "plain": ([0, 3, 5, 8, 10], [1, 2, 3, 0, 2, 0, 1, 3, 0, 2]),
    "self_loops": ([0, 4, 7, 10, 12], [0, 1, 2, 3, 0, 1, 2, 0, 1, 3, 0, 2]),
}
KNOWN_COUNTS = [2, 1, 2, 1]
KNOWN_T = 2
