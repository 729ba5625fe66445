"""Checker of grx_pagerank: the iteration of essentials_amd/csrc/clients.hxx (pr_problem_t, pr_enactor_t,
pr_pull_enactor_t -- the reference's pr.hxx:64-178) restated in numpy float64 for a FIXED number of
iterations, with a first-order bound on what a float32 run of the same iteration may differ by at every
vertex, an emulation of that float32 run (with deliberate defects) to prove the bound on the CPU, and
the small graphs the device tests run on.  numpy only: no GPU, no oracle/.  The checker, never the thing
shipped.

The bound.  u = 2**-24.  Every float32 operation returns its exact result times (1 + d), |d| <= u.
Every quantity here is non-negative, so every partial sum is at most the total and the bound holds for
ANY order of the adds (float atomics, shuffles, chunks) and with or without fma contraction (fewer
roundings).  E is carried beside p:

    tot[v]   = sum of v's out-weights;  scale[v] = alpha / tot[v] (0 when tot[v] == 0: dangling)
               relative error rs[v] = (outdeg(v) + 2) u   (outdeg - 1 adds, the division, one spare)
    p = 1/n, E = u p
    per iteration
      D    = alpha * sum of p over the dangling vertices
      ED   = alpha * sum of E over them + (n_dangling + log2 n + 4) u D
      base = (1 - alpha + D) / n,  Eb = ED / n + 4 u base
      per edge    term = p[src] scale[src] w,  Et = E[src] scale[src] w + term (rs[src] + 3 u)
      per vertex  S = base + sum of its in-terms,  A = Eb + sum of their Et,
                  E' = A + (indeg + 1) u (S + A),  p' = S
    allowed = 2 E

The factor 2 covers the second-order terms (under 1 % while indeg * u * T < 1e-2, asserted) and this
float64 loop's own rounding.  3u, 4u and the +2 each carry one unit over the operation count.
"""
import numpy as np

U = 2.0 ** -24


def _arrays(ap, aj, aw):
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    dst = np.asarray(aj, np.int64)[: len(src)]
    w32 = np.asarray(aw, np.float32)[: len(src)]
    return n, src, dst, w32


def in_degrees(ap, aj):
    n = len(ap) - 1
    return np.bincount(np.asarray(aj, np.int64)[: int(ap[-1])], minlength=n)[:n]


def reference(ap, aj, aw, alpha, T):
    """-> (p, allowed), float64 [n]: the ranks after exactly T iterations and the largest |got - p| a
    float32 run of the same T iterations may show at each vertex."""
    n, src, dst, w32 = _arrays(ap, aj, aw)
    w = w32.astype(np.float64)
    assert n >= 1 and T >= 1
    assert (w >= 0).all(), "negative weight: the bound needs non-negative terms"
    alpha32 = float(np.float32(alpha))
    outdeg = np.bincount(src, minlength=n)[:n]
    indeg = np.bincount(dst, minlength=n)[:n]
    assert (indeg.max() if n else 0) * U * T < 1e-2, "second-order terms no longer negligible"
    tot = np.bincount(src, weights=w, minlength=n)[:n]
    dangling = tot == 0
    scale = np.where(dangling, 0.0, alpha32 / np.where(dangling, 1.0, tot))
    rs = (outdeg + 2) * U
    n_dangling = int(dangling.sum())
    p = np.full(n, 1.0 / n)
    E = U * p
    sw = scale[src] * w
    for _ in range(T):
        D = alpha32 * p[dangling].sum()
        ED = alpha32 * E[dangling].sum() + (n_dangling + np.log2(n) + 4) * U * D
        base = (1.0 - alpha32 + D) / n
        Eb = ED / n + 4 * U * base
        term = p[src] * sw
        Et = E[src] * sw + term * (rs[src] + 3 * U)
        if (term > 0).any():
            assert term[term > 0].min() > 2.0 ** -100, "a term near float32 underflow"
        S = base + np.bincount(dst, weights=term, minlength=n)[:n]
        A = Eb + np.bincount(dst, weights=Et, minlength=n)[:n]
        E = A + (indeg + 1) * U * (S + A)
        p = S
    return p, 2.0 * E


def iterations_to_tolerance(ap, aj, aw, alpha, tol, limit=10000):
    """The iteration after which the float64 loop itself stops: the first (>= 1) whose largest change
    max |p' - p| is below float32(tol) -- is_converged() of the enactors."""
    n, src, dst, w32 = _arrays(ap, aj, aw)
    w = w32.astype(np.float64)
    alpha32, tol32 = float(np.float32(alpha)), float(np.float32(tol))
    tot = np.bincount(src, weights=w, minlength=n)[:n]
    dangling = tot == 0
    sw = (np.where(dangling, 0.0, alpha32 / np.where(dangling, 1.0, tot)))[src] * w
    p = np.full(n, 1.0 / n)
    for t in range(1, limit + 1):
        new = (1.0 - alpha32 + alpha32 * p[dangling].sum()) / n + np.bincount(dst, weights=p[src] * sw,
                                                                                minlength=n)[:n]
        err = np.abs(new - p).max()
        p = new
        if err < tol32:
            return t
    return limit


def ratio(got, p, allowed):
    """|got - p| / allowed per vertex."""
    return np.abs(np.asarray(got).astype(np.float64) - p) / allowed


# ---------------------------------------------------------------------------
# the float32 stand-in for the device, and its deliberate defects
# ---------------------------------------------------------------------------
def emulate(ap, aj, aw, alpha, T, rng, fault=None):
    """The same T iterations in float32 numpy, the adds in a random order drawn anew every iteration
    (np.add.at over a permutation of the edges): what a correct device run may return.  fault, one of

      ("drop", edges)        those edge ids (positions in aj) left out of the sums
      ("twice", edges)       those edges counted twice
      ("transpose",)         every vertex sums over its OUT-row instead of its in-row
      ("no_dangling",)       the dangling mass omitted
      ("zero_row_live",)     a row whose weights are all 0 not counted as dangling
      ("scatter", frm)       ranks computed in another numbering (frm[v] = v's id there) and handed
                             back as out[frm[v]] = own[v] instead of out[v] = own[frm[v]]
      ("iterations", d)      T + d iterations
      ("stale", block)       the sources of edges [256 block, 256 block + 256) read from the rank being
                             written instead of the previous one
    """
    f32 = np.float32
    n, src, dst, w = _arrays(ap, aj, aw)
    m = len(src)
    kind = fault[0] if fault else None
    a = f32(alpha)
    one = f32(1.0)
    outdeg = np.bincount(src, minlength=n)[:n]
    tot = np.zeros(n, f32)
    order = rng.permutation(m)
    np.add.at(tot, src[order], w[order])
    dangling = tot == 0
    with np.errstate(divide="ignore"):
        scale = np.where(dangling, f32(0), a / np.where(dangling, one, tot)).astype(f32)
    counted = dangling if kind != "zero_row_live" else outdeg == 0
    if kind == "iterations":
        T = T + fault[1]
    p = np.full(n, f32(1.0 / n), f32)
    nf = f32(n)
    for _ in range(T):
        if kind == "no_dangling":
            D = f32(0)
        else:
            give = (a * p[counted]).astype(f32)
            acc = np.zeros(1, f32)
            np.add.at(acc, np.zeros(len(give), np.int64), give[rng.permutation(len(give))])
            D = acc[0]
        base = f32(f32(f32(one - a) + D) / nf)
        new = np.full(n, base, f32)
        s, d = (dst, src) if kind == "transpose" else (src, dst)
        term = ((p[s] * scale[s]).astype(f32) * w).astype(f32)
        keep = np.ones(m, bool)
        late = np.zeros(m, bool)
        if kind == "drop":
            keep[np.asarray(fault[1], np.int64)] = False
        if kind == "stale":
            late[256 * fault[1]: 256 * fault[1] + 256] = True
        order = rng.permutation(m)
        order = order[keep[order] & ~late[order]]
        if kind == "twice":
            order = rng.permutation(np.concatenate([order, np.asarray(fault[1], np.int64)]))
        np.add.at(new, d[order], term[order])
        if kind == "stale":
            e = np.flatnonzero(late)
            np.add.at(new, d[e], ((new[s[e]] * scale[s[e]]).astype(f32) * w[e]).astype(f32))
        p = new
    if kind == "scatter":
        frm = np.asarray(fault[1], np.int64)
        own = np.empty(n, f32)
        own[frm] = p          # the run's numbering
        out = np.empty(n, f32)
        out[frm] = own        # the defect; out = own[frm] would be p again
        return out
    return p


# ---------------------------------------------------------------------------
# graphs: deterministic, (ap, aj, aw) int32 / int32 / float32, weights integer-valued in [0, 64]
# ---------------------------------------------------------------------------
def csr(n, src, dst, w):
    """CSR of the edges in the order given within every row (stable): repeats and loops stay."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    w = np.asarray(w, np.float64)
    assert len(src) == len(dst) == len(w)
    assert ((w >= 0) & (w <= 64) & (w == np.round(w))).all()
    order = np.argsort(src, kind="stable")
    ap = np.zeros(n + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(src, minlength=n)[:n])
    return ap.astype(np.int32), dst[order].astype(np.int32), w[order].astype(np.float32)


def in_rows(ap, aj):
    """(tp, edge): the edge ids (positions in aj) grouped by destination, CSR order within a
    destination -- the order of the engine's destination-sorted list and of an attached transpose."""
    n = len(ap) - 1
    dst = np.asarray(aj, np.int64)
    edge = np.argsort(dst, kind="stable")
    tp = np.zeros(n + 1, np.int64)
    tp[1:] = np.cumsum(np.bincount(dst, minlength=n)[:n])
    return tp, edge


HUB_RICH = (0, 15, 16, 255, 256, 2047, 2048)
HUB_SIZES = (255, 256, 257, 2047, 2048, 2049, 4097)


def hub_rich(m):
    return sorted({j for j in HUB_RICH + (m - 1,) if 0 <= j < m})


def hub(m, rich=None):
    """Two hubs (vertices 0 and 1) that each receive from every one of m leaves (vertices 2 .. m + 1);
    vertex m + 2 is isolated.  Leaf j sends w_j to hub 0 and 65 - w_j to hub 1, so every leaf hands out
    the same total.  Leaf ids rise with j, so leaf j sits at position j of hub 0's in-row (m entries:
    around RED_HUB = 256 and RED_CHUNK = 2048 for the sizes in HUB_SIZES).  w_j is 64 at the positions in
    `rich` and 1 elsewhere: on hub 0 a rich position outweighs 63 others, so losing it is decisive
    even where 1/m is close to m u.  Three leaves just before the last one have w_j = 0 -- a
    zero-weight edge into hub 0 -- and split their 65 over two parallel edges into hub 1, whose in-row
    is therefore m + 3 long and agrees with hub 0's in the positions before them.  Each hub has one
    feedback edge, to one of those three: the mass a hub hands back then returns through hub 1's row
    only, and the rich positions of hub 0's row stay decisive after the first iteration as well."""
    rich = hub_rich(m) if rich is None else sorted(rich)
    assert m >= 16
    plain = [j for j in range(m - 2, -1, -1) if j not in rich]
    zero = sorted(plain[:3])
    feedback = zero[:2]
    src, dst, w = [0, 1], [2 + feedback[0], 2 + feedback[1]], [8, 8]
    for j in range(m):
        if j in zero:
            src += [2 + j] * 3
            dst += [0, 1, 1]
            w += [0, 32, 33]
        else:
            wj = 64 if j in rich else 1
            src += [2 + j] * 2
            dst += [0, 1]
            w += [wj, 65 - wj]
    return csr(m + 3, src, dst, w)


def hub_edge(ap, aj, j, which=0):
    """Edge id of leaf j's (first) edge into hub `which`."""
    row = np.arange(int(ap[2 + j]), int(ap[3 + j]))
    return int(row[np.asarray(aj)[row] == which][0])


SHORT_DEGREES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255)


def short_rows():
    """Vertex i < 13 has in-degree SHORT_DEGREES[i] and out-degree SHORT_DEGREES[(i + 5) % 13]: around
    the RED_GROUP = 16 stripes and the 64-lane wavefront, 255 just below RED_HUB = 256.  Its in-edges
    come from, and its out-edges go to, distinct ones of 300 further vertices, so ranks circulate
    and n = 313 is no power of two.  Directed."""
    k, fill = len(SHORT_DEGREES), 300
    src, dst, w = [], [], []
    e = 0
    for i, deg in enumerate(SHORT_DEGREES):
        for t in range(deg):                                   # in-edges of i
            src.append(k + (37 * i + 7 * t) % fill)
            dst.append(i)
            w.append(16 + (5 * e) % 49)
            e += 1
    for i in range(k):
        for t in range(SHORT_DEGREES[(i + 5) % k]):            # out-edges of i
            src.append(i)
            dst.append(k + (53 * i + 11 * t + 3) % fill)
            w.append(16 + (5 * e) % 49)
            e += 1
    return csr(k + fill, src, dst, w)


RUN_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257)
RUN_OFFSETS = (0, 1, 63)


def runs_layout():
    """In-degrees by vertex id, and (vertex, start, length) of the runs under test."""
    indeg, tested, pos = [], [], 0
    for off in RUN_OFFSETS:
        for length in RUN_LENGTHS:
            pad = (off - pos) % 64
            if pad:
                indeg.append(pad)
                pos += pad
            if len(indeg) % 5 == 2:
                indeg.append(0)                                # vertices nobody points at, in between
            tested.append((len(indeg), pos, length))
            indeg.append(length)
            pos += length
    if pos % 256 == 0:
        indeg.append(1)
    return indeg, tested


def runs():
    """A directed graph whose destination-sorted edge list holds, for every length in RUN_LENGTHS, runs
    of one destination that start at offsets 0, 1 and 63 of a 64-lane wavefront (filler runs pad in
    between); runs straddle positions 64 and 256 (wavefront and BLOCK of expand_kernel) and the list
    length is no multiple of 256.  The sources are spread over all n = 331 vertices."""
    indeg, _ = runs_layout()
    n = 331
    assert len(indeg) < n
    dst = np.repeat(np.arange(len(indeg)), indeg)
    e = np.arange(len(dst))
    src = (e * 7 + dst * 3) % n
    w = 8 + (e * 5) % 57
    return csr(n, src, dst, w)


def dangling():
    """n = 1000: every third vertex has no out-edges, row 1 has five edges whose weights are all 0 (so
    it is dangling too: scale == 0), vertex 2 has a self loop and vertex 4 two parallel edges to 5."""
    n = 1000
    src, dst, w = [], [], []
    for v in range(n):
        if v % 3 == 0:
            continue
        if v == 1:
            for t in range(5):
                src.append(1); dst.append(10 + 7 * t); w.append(0)
            continue
        for t in range(1 + v % 7):
            src.append(v)
            dst.append((37 * v + 101 * t + 11) % n)
            w.append(1 + (v + 3 * t) % 64)
    src += [2, 4, 4]
    dst += [2, 5, 5]
    w += [9, 3, 4]
    for t in range(12):                                        # row 1 holds some mass to strand
        src.append(50 + 3 * t); dst.append(1); w.append(40)
    return csr(n, src, dst, w)


def random_directed(n=1000, degree=8, seed=12345):
    """A plain directed graph: n * degree edges from a linear congruential generator."""
    x = seed
    src, dst, w = [], [], []
    for _ in range(n * degree):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        src.append((x >> 33) % n)
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        dst.append((x >> 33) % n)
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        w.append(1 + (x >> 33) % 64)
    return csr(n, src, dst, w)


def tiny(n):
    """n = 1: a self loop; n = 2: 0 -> 1 (1 dangling); n = 3: 0 -> 1, 0 -> 2, 1 -> 2, 2 -> 0."""
    edges = {1: [(0, 0, 3)], 2: [(0, 1, 2)], 3: [(0, 1, 1), (0, 2, 2), (1, 2, 5), (2, 0, 64)]}[n]
    s, d, w = zip(*edges)
    return csr(n, s, d, w)


def edgeless(n=5):
    return csr(n, [], [], [])


def degree_sorted(ap):
    """frm[v]: v's id in the numbering that sorts vertices by falling out-degree (stable)."""
    order = np.argsort(-np.diff(np.asarray(ap, np.int64)), kind="stable")
    frm = np.empty(len(order), np.int64)
    frm[order] = np.arange(len(order))
    return frm


def cases():
    """name -> (ap, aj, aw): every graph built here; all are directed."""
    out = {f"hub{m}": hub(m) for m in HUB_SIZES}
    out.update(short_rows=short_rows(), runs=runs(), dangling=dangling(), random=random_directed())
    for n in (1, 2, 3):
        out[f"tiny{n}"] = tiny(n)
    out["edgeless"] = edgeless()
    return out
