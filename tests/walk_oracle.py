"""Oracle of grx_random_walk: the definition of include/essentials_amd.h followed literally, one walk
and one step at a time, in numpy and Python integers.  The checker, never the thing shipped."""
import numpy as np

M64 = (1 << 64) - 1
BLOCK = 64
MAX_ATTEMPTS = 1024


def mix64(x):
    """The splitmix64 finaliser of x + 0x9E3779B97F4A7C15 (grx_graph_rmat's mix64)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, i, t, j):
    """r(i, t, j)."""
    return mix64((mix64((seed & M64) ^ mix64(i)) + (t << 32) + j) & M64)


def u24(r):
    return np.float32(r >> 40) * np.float32(2.0 ** -24)


def prefix(weights):
    """c of one row: float32 cumsum per block of 64, the block bases added in block order."""
    w = np.asarray(weights, np.float32)
    c = np.empty(len(w), np.float32)
    base = np.float32(0)
    for lo in range(0, len(w), BLOCK):
        l = np.cumsum(w[lo:lo + BLOCK], dtype=np.float32)
        c[lo:lo + BLOCK] = base + l
        base = np.float32(base + l[-1])
    return c


def pick_uniform(r, d):
    return ((r >> 32) * d) >> 32


def pick_weighted(c, r):
    W = c[-1]
    x = np.float32(u24(r) * W)
    above = np.flatnonzero(c > x)
    return int(above[0]) if len(above) else int(np.flatnonzero(c == W)[0])


def ratios(p, q):
    """(ret, adj, far) in float32."""
    one = np.float32(1)
    ip, iq = one / np.float32(p), one / np.float32(q)
    m = max(ip, one, iq)
    return np.float32(ip / m), np.float32(one / m), np.float32(iq / m)


def random_walk(ap, aj, ax=None, starts=None, length=1, seed=0, weighted=False, p=1.0, q=1.0, cap=MAX_ATTEMPTS):
    """-> dict: walks [count, length + 1] int32 (-1 behind a dead end), iterations (the longest walk's
    steps), full (walks of `length` steps), steps, attempts, slots (walks that took step t, for
    t = 1..min(iterations, 64)) and launches (the walker, 3 for the prefix array, 2 for sorted rows)."""
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    n = len(ap) - 1
    starts = np.arange(n) if starts is None else np.atleast_1d(np.asarray(starts, np.int64))
    ret, adj, far = ratios(p, q)
    second = not (np.float32(p) == 1 and np.float32(q) == 1)
    rows = {}    # v -> prefix array
    member = {}  # v -> set of the columns of row v

    def c_of(v):
        if v not in rows:
            rows[v] = prefix(ax[ap[v]:ap[v + 1]])
        return rows[v]

    walks = np.full((len(starts), length + 1), -1, np.int32)
    taken = np.zeros(len(starts), np.int64)
    attempts = 0
    for i, start in enumerate(starts):
        v, prev = int(start), None
        walks[i, 0] = v
        for t in range(1, length + 1):
            lo, d = int(ap[v]), int(ap[v + 1] - ap[v])
            if d == 0 or (weighted and not c_of(v)[-1] > 0):
                break
            a = 0
            while True:
                r = draw(seed, i, t, 2 * a)
                k = pick_weighted(c_of(v), r) if weighted else pick_uniform(r, d)
                x = int(aj[lo + k])
                attempts += 1
                if t == 1:
                    break
                if prev not in member:
                    member[prev] = set(aj[ap[prev]:ap[prev + 1]].tolist())
                ratio = ret if x == prev else adj if x in member[prev] else far
                if ratio == 1 or u24(draw(seed, i, t, 2 * a + 1)) < ratio:
                    break
                a += 1
                if a >= cap:  # `cap` rejected attempts: the last candidate is taken
                    break
            prev, v = v, x
            walks[i, t] = v
            taken[i] = t
    iterations = int(taken.max()) if len(taken) else 0
    edges = length > 0 and len(aj) > 0
    return {"walks": walks, "iterations": iterations, "full": int((taken == length).sum()),
            "steps": int(taken.sum()), "attempts": attempts,
            "slots": [int((taken >= t).sum()) for t in range(1, min(iterations, 64) + 1)],
            "launches": 1 + (3 if weighted and edges else 0) + (2 if second and edges and length > 1 else 0)}


def csr(n, edges, weights=None):
    """CSR (int32 ap, aj, float32 ax) of directed `edges` ([m, 2]) in the order given per row: repeats
    and loops stay; weight 1 when none are given."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.ones(len(e), np.float32) if weights is None else np.asarray(weights, np.float32)
    order = np.argsort(e[:, 0], kind="stable")
    ap = np.zeros(n + 1, np.int64)
    np.add.at(ap, e[:, 0] + 1, 1)
    return np.cumsum(ap).astype(np.int32), e[order, 1].astype(np.int32), w[order]


def mtx_csr(path):
    """Symmetric CSR of a coordinate Matrix Market pattern file without self loops, in the loader's row
    order: every line gives (u, v) then (v, u), and rows keep the order of the lines.  Weights 1."""
    rows = [l.split() for l in open(path) if not l.startswith("%")]
    e = np.asarray([(int(r[0]) - 1, int(r[1]) - 1) for r in rows[1:]], np.int64)
    assert (e[:, 0] != e[:, 1]).all()
    return csr(int(rows[0][0]), np.stack([e, e[:, ::-1]], axis=1).reshape(-1, 2))


def chi_square(observed, probability):
    """Pearson's statistic of counts against cell probabilities (cells of probability 0 must be empty)
    -> (statistic, degrees of freedom)."""
    observed, probability = np.asarray(observed, np.float64), np.asarray(probability, np.float64)
    live = probability > 0
    assert observed[~live].sum() == 0
    expected = observed.sum() * probability[live] / probability[live].sum()
    return float(((observed[live] - expected) ** 2 / expected).sum()), int(live.sum()) - 1
