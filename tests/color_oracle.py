"""Greedy colouring of a symmetric CSR in largest-degree-first order, in plain numpy (the GPU machine
may lack scipy and networkx).  deg(v) is the length of row v as given (a repeated entry counts each
time, a self loop once); key(v) = (deg(v) << 32) | fmix32(v); u precedes v when u != v, u appears in
row v and key(u) > key(v); color[v] is the smallest integer >= 0 that no predecessor of v has.
`greedy` is that definition, one vertex at a time in descending key; `colouring` gets the same
answer generation by generation, vectorised, and is what the GPU tests compare against."""
import numpy as np

from kcore_oracle import simple_csr  # noqa: F401  (re-exported for the tests)
from tc_oracle import csr, mtx_csr  # noqa: F401  (re-exported for the tests)


def fmix32(v):
    """The 32-bit finaliser on unsigned ids (an array or an int) -> uint64 values below 2^32."""
    h = np.asarray(v).astype(np.uint64) & np.uint64(0xffffffff)
    m = np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & m
    h ^= h >> np.uint64(16)
    return h


def keys(ap):
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    return (np.diff(ap).astype(np.uint64) << np.uint64(32)) | fmix32(np.arange(n))


def greedy(ap, aj):
    """int32 colours: sequential greedy colouring, vertices in descending key."""
    ap = np.asarray(ap, np.int64)
    aj = np.asarray(aj, np.int64)
    n = len(ap) - 1
    key = keys(ap)
    color = np.full(n, -1, np.int32)
    for v in np.argsort(key)[::-1]:
        row = aj[ap[v]:ap[v + 1]]
        # a coloured neighbour was taken earlier, so it has the larger key; v itself is uncoloured
        taken = set(color[row].tolist())
        c = 0
        while c in taken:
            c += 1
        color[v] = c
    return color


def colouring(ap, aj):
    """(int32 colours, num_colors = 1 + the largest colour or 0 for V == 0, depth of the priority
    DAG = the number of generations)."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    if n == 0:
        return np.zeros(0, np.int32), 0, 0
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    key = keys(ap)
    # the entries (v, u) where u precedes v, sorted by v: pred[first[v]:first[v + 1]]
    before = (row != col) & (key[col] > key[row])
    prow, pred = row[before], col[before]
    first = np.zeros(n + 1, np.int64)
    first[1:] = np.cumsum(np.bincount(prow, minlength=n))
    # and where v precedes u, sorted by v: the vertices a coloured v tells
    after = (row != col) & (key[col] < key[row])
    arow, succ = row[after], col[after]
    afirst = np.zeros(n + 1, np.int64)
    afirst[1:] = np.cumsum(np.bincount(arow, minlength=n))
    pending = np.diff(first)
    color = np.full(n, -1, np.int64)
    ready = np.flatnonzero(pending == 0)
    depth = 0
    while len(ready):
        depth += 1
        lens = first[ready + 1] - first[ready]
        total = int(lens.sum())
        color[ready] = 0
        if total:
            slot = np.repeat(np.arange(len(ready)), lens)
            at = np.repeat(first[ready] - (np.cumsum(lens) - lens), lens) + np.arange(total)
            # sorted distinct (ready vertex, predecessor colour) pairs; rank = position in its vertex
            pair = np.unique(slot * (n + 1) + color[pred[at]])
            s, c = pair // (n + 1), pair % (n + 1)
            start = np.searchsorted(s, np.arange(len(ready)))
            rank = np.arange(len(pair)) - start[s]
            # mex = the first rank whose colour differs from it, or the number of pairs
            mex = np.bincount(s, minlength=len(ready)).astype(np.int64)
            gap = c != rank
            np.minimum.at(mex, s[gap], rank[gap])
            color[ready] = mex
        lens = afirst[ready + 1] - afirst[ready]
        total = int(lens.sum())
        if not total:
            break
        at = np.repeat(afirst[ready] - (np.cumsum(lens) - lens), lens) + np.arange(total)
        told = succ[at]
        np.subtract.at(pending, told, 1)
        ready = np.unique(told[pending[told] == 0])
    assert (color >= 0).all()
    return color.astype(np.int32), int(color.max()) + 1, depth


def predecessors(ap, aj):
    """Distinct predecessors per vertex (int64)."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    key = keys(ap)
    before = (row != col) & (key[col] > key[row])
    pair = np.unique(row[before] * max(n, 1) + col[before])
    return np.bincount(pair // max(n, 1), minlength=n)


def is_proper(ap, aj, color):
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    color = np.asarray(color)
    return bool((color[row] != color[col])[row != col].all())


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


def _by_key(n, edges, both=True):
    """Vertex ids in descending key for a hand-written graph."""
    ap, _ = csr(n, np.asarray(edges, np.int64).reshape(-1, 2), symmetric=both)
    return np.argsort(keys(ap))[::-1]


def _known():
    """name -> (V, edge list, add both directions, colours).  The answers are written by hand from
    the structure; where they depend on the hash order of equal degrees they are stated in terms
    of that order (the rank of a vertex among its equals), never computed by a colouring."""
    k = {}
    for n in (2, 5, 12):  # a clique: equal degrees, so the vertex of hash rank r gets colour r
        order = _by_key(n, _clique(0, n))
        want = np.empty(n, np.int64)
        want[order] = np.arange(n)
        k[f"complete{n}"] = (n, _clique(0, n), True, want.tolist())
    k["star"] = (30, [(0, i) for i in range(1, 30)], True, [0] + [1] * 29)
    k["star_hub_last"] = (30, [(29, i) for i in range(29)], True, [1] * 29 + [0])
    k["isolated"] = (9, [], True, [0] * 9)
    k["empty"] = (0, [], True, [])
    k["only_a_self_loop"] = (3, [(0, 0)], False, [0, 0, 0])
    # one edge stored many times, and a self loop on the vertex of larger degree: two colours
    k["repeats_and_a_self_loop"] = (2, [(0, 1)] * 7 + [(0, 0)], True, [0, 1])
    # a triangle whose degrees are made distinct by pendant vertices: 0 (deg 5) first, then 1
    # (deg 4), then 2 (deg 3); every pendant vertex sees only its hub
    tri = [(0, 1), (1, 2), (2, 0), (0, 3), (0, 4), (0, 5), (1, 6), (1, 7), (2, 8)]
    k["triangle_with_pendants"] = (9, tri, True, [0, 1, 2, 1, 1, 1, 0, 0, 0])
    # K5 on 0..4 with a tail 4-5-6-7: 4 has the largest degree; 5 (deg 2) follows 4 and precedes
    # or follows 6 (deg 2) by hash; 7 (deg 1) is last.  The clique's other members by hash rank.
    edges = _clique(0, 5) + [(4, 5), (5, 6), (6, 7)]
    order = [int(v) for v in _by_key(8, edges)]
    want = [0] * 8
    want[4] = 0
    for r, v in enumerate([v for v in order if v < 4]):
        want[v] = r + 1
    if order.index(5) < order.index(6):
        want[5], want[6], want[7] = 1, 0, 1
    else:  # 6 first: it sees nobody coloured; 5 then sees 4 (0) and 6 (0)
        want[6], want[5], want[7] = 0, 1, 1
    k["k5_pendant_path"] = (8, edges, True, want)
    return k


KNOWN = _known()


def known_csr(name):
    n, edges, both, want = KNOWN[name]
    ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2), symmetric=both)
    return ap, aj, np.asarray(want, np.int32)
