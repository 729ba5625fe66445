"""Oracle of grx_bfs_multi: a numpy level-synchronous BFS per source over (ap, aj), nothing shared
between the sources.  The checker, never the thing shipped."""
import numpy as np

UNREACHED = 2**31 - 1
BATCH = 64


def csr(n, edges, symmetric=True):
    """CSR (int32 ap, aj) of `edges` ([m, 2] vertex pairs) as given: repeats and loops stay."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if symmetric and len(e):
        e = np.concatenate([e, e[:, ::-1]])
    order = np.argsort(e[:, 0], kind="stable")
    e = e[order]
    ap = np.zeros(n + 1, np.int64)
    np.add.at(ap, e[:, 0] + 1, 1)
    return np.cumsum(ap).astype(np.int32), e[:, 1].astype(np.int32)


def mtx_csr(path):
    """Symmetric CSR of a coordinate Matrix Market file (pattern or valued, 1-based)."""
    rows = [l.split() for l in open(path) if not l.startswith("%")]
    n = int(rows[0][0])
    e = np.asarray([(int(r[0]) - 1, int(r[1]) - 1) for r in rows[1:]], np.int64)
    return csr(n, e)


def single_source(ap, aj, source):
    """Depths of one search: frontier by frontier, out-entries as given."""
    n = len(ap) - 1
    depth = np.full(n, UNREACHED, np.int64)
    depth[source] = 0
    frontier = np.asarray([source], np.int64)
    level = 0
    while len(frontier):
        lo, hi = ap[frontier].astype(np.int64), ap[frontier + 1].astype(np.int64)
        d = hi - lo
        if d.sum() == 0:
            break
        at = np.repeat(lo - np.concatenate([[0], np.cumsum(d)[:-1]]), d) + np.arange(d.sum())
        seen = np.unique(aj[at].astype(np.int64))
        frontier = seen[depth[seen] == UNREACHED]
        level += 1
        depth[frontier] = level
    return depth


def multi_source(ap, aj, sources=None):
    """-> dict: depths [count, V] int32 (UNREACHED where unreached), reached / depth_sum (int64) and
    eccentricity (int32) per source, levels (per batch of 64: 1 + the largest eccentricity in it),
    active (of the first batch: per level, the vertices that have that depth for some source),
    degrees (per batch: per level, the out-degrees of the level's active vertices summed) and traversed
    (their sum over batches and levels)."""
    ap, aj = np.asarray(ap), np.asarray(aj)
    n = len(ap) - 1
    sources = np.arange(n) if sources is None else np.atleast_1d(np.asarray(sources, np.int64))
    count = len(sources)
    depths = np.full((count, n), UNREACHED, np.int32)
    for i, s in enumerate(sources):
        depths[i] = single_source(ap, aj, int(s))
    finite = depths != UNREACHED
    reached = finite.sum(1).astype(np.int64)
    depth_sum = np.where(finite, depths, 0).astype(np.int64).sum(1)
    eccentricity = np.where(finite, depths, -1).max(1).astype(np.int32) if n else np.zeros(count, np.int32)
    degree = np.diff(ap).astype(np.int64)
    levels, active, degrees = [], [], []
    for first in range(0, count, BATCH):
        rows = depths[first:first + BATCH]
        top = int(eccentricity[first:first + BATCH].max()) if n else -1
        levels.append(top + 1)
        degrees.append([])
        for level in range(top + 1):
            on = (rows == level).any(0)
            degrees[-1].append(int(degree[on].sum()))
            if first == 0:
                active.append(int(on.sum()))
    return {"depths": depths, "reached": reached, "depth_sum": depth_sum, "eccentricity": eccentricity,
            "levels": levels, "active": active, "degrees": degrees, "traversed": sum(sum(d) for d in degrees)}
