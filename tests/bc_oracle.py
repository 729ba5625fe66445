"""What the betweenness-centrality tests share (numpy only): small graph builders whose rows sit at
grx_bc's own thresholds, a float64 Brandes with a per-vertex count of the float32 roundings that
can touch bc[v], and a float32 Brandes in the kernel's arithmetic for the graphs on which the order
of the additions cannot matter.

The kernels (include/gunrock/hip/kernels/bc_kernels.hxx) compute, per source and level,
    forward:   sigma[v] = sum of sigma[u] over the in-edges from one level up;  rho[v] = 1 / sigma[v]
    backward:  sum = sum of rho[w] over the out-edges to one level down;  delta[u] = sigma[u] * sum;
               rho[u] = fma(sigma[u], sum, 1) / sigma[u];  bc[u] += 0.5 * delta[u]
with correctly rounded divisions.  Every quantity is non-negative.  A sum of c non-negative terms
taken in ANY order, zeros for empty lanes and chunks included, is within (c - 1) roundings of the
exact sum of its terms on top of the worst term's own; a product or a quotient adds one.  That is
the count K of brandes64, and gamma(K) = K u / (1 - K u), u = 2^-24, the relative bound."""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)

# the kernels' thresholds (bc_kernels.hxx) and the row lengths around them
BC_GROUP, BC_HUB, BC_CHUNK = 16, 256, 2048
BOUNDARY_LENGTHS = (255, 256, 257, 2047, 2048, 2049, 4096, 4097)


def csr(n, edges, symmetric=True):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if symmetric:
        e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    ap = np.zeros(n + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(e[:, 0], minlength=n))
    return ap.astype(np.int32), e[:, 1].astype(np.int32)


def gamma(K):
    K = np.asarray(K, np.float64)
    return K * U / (1.0 - K * U)


def chunks_of(in_deg, out_deg):
    """bc_chunks_of: the chunk slots of a row."""
    deg = max(int(in_deg), int(out_deg))
    return -(-deg // BC_CHUNK) if deg >= BC_HUB else 0


# ---------------------------------------------------------------------------
# the search both references share
# ---------------------------------------------------------------------------
class LevelGraph:
    def __init__(self, ap, aj):
        self.ap = np.asarray(ap, np.int64)
        self.n = len(self.ap) - 1
        self.dst = np.asarray(aj, np.int64)
        self.src = np.repeat(np.arange(self.n), np.diff(self.ap))

    def search(self, s):
        """(depth, levels): levels[d] = (u, w) of the edges from depth d to depth d + 1, in edge
        order, every parallel edge on its own."""
        depth = np.full(self.n, -1, np.int64)
        depth[s] = 0
        frontier = np.array([s], np.int64)
        d = 0
        while True:
            lo, cnt = self.ap[frontier], self.ap[frontier + 1] - self.ap[frontier]
            at = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
            ends = self.dst[at]
            frontier = np.unique(ends[depth[ends] < 0])
            if not len(frontier):
                break
            d += 1
            depth[frontier] = d
        e = np.flatnonzero((depth[self.src] >= 0) & (depth[self.dst] == depth[self.src] + 1))
        e = e[np.argsort(depth[self.src[e]], kind="stable")]
        cut = np.searchsorted(depth[self.src[e]], np.arange(d + 1))
        return depth, [(self.src[e[cut[i]:cut[i + 1]]], self.dst[e[cut[i]:cut[i + 1]]]) for i in range(d)]


def _is_float32(x):
    with np.errstate(over="ignore"):
        return bool((x.astype(np.float32).astype(np.float64) == x).all())


# ---------------------------------------------------------------------------
# float64 Brandes with the rounding count
# ---------------------------------------------------------------------------
def brandes64(ap, aj, sources, details=False):
    """(bc, reached, edges, levels, K).  bc[v] = 0.5 * sum over sources of delta_s(v) in float64,
    level-synchronous, every parallel edge a path of its own.  reached / edges / levels are what
    grx_stats reports, each summed over sources: reached vertices, their out-degrees, and 1 + the
    last depth.  K[v]: the float32 roundings that can touch bc[v] (see the module's docstring):
        Ksigma[v] = max Ksigma[u] + c - 1 over the c contributing in-edges;
        Krho = Ksigma + 1 at the last level;
        Kdelta[u] = max Krho[w] + c - 1 + Ksigma[u] + 1 over the c contributing out-edges (0 when
        none contributes);  Krho[u] = Kdelta[u] + Ksigma[u] + 2;
        Kbc[v] = max(Kbc[v], Kdelta[v]) + 1 for every source whose delta(v) is not zero.
    With details=True a sixth value says whether every intermediate was a float32 value."""
    G = LevelGraph(ap, aj)
    n = G.n
    outdeg = np.diff(G.ap)
    bc = np.zeros(n)
    K = np.zeros(n, np.int64)
    reached = edges = levels = 0
    all32 = True
    for s in sources:
        depth, lv = G.search(int(s))
        sigma = np.zeros(n)
        sigma[s] = 1.0
        Ks = np.zeros(n, np.int64)
        for u, w in lv:
            np.add.at(sigma, w, sigma[u])
            c = np.bincount(w, minlength=n)
            worst = np.zeros(n, np.int64)
            np.maximum.at(worst, w, Ks[u])
            Ks = np.where(c > 0, worst + c - 1, Ks)
        delta = np.zeros(n)
        Kd = np.zeros(n, np.int64)
        Kr = Ks + 2
        Kr[depth == len(lv)] = Ks[depth == len(lv)] + 1
        for u, w in lv[::-1]:
            one_plus = 1.0 + delta[w]
            ratio = sigma[u] / sigma[w]
            term = ratio * one_plus
            np.add.at(delta, u, term)
            all32 = all32 and _is_float32(one_plus) and _is_float32(ratio) and _is_float32(term)
            c = np.bincount(u, minlength=n)
            worst = np.zeros(n, np.int64)
            np.maximum.at(worst, u, Kr[w])
            Kd = np.where(c > 0, worst + c - 1 + Ks + 1, Kd)
            Kr = np.where(c > 0, Kd + Ks + 2, Kr)
        delta[s] = 0.0
        bc += delta
        all32 = all32 and _is_float32(sigma) and _is_float32(delta) and _is_float32(bc)
        K = np.where(delta > 0, np.maximum(K, Kd) + 1, K)
        reached += int((depth >= 0).sum())
        edges += int(outdeg[depth >= 0].sum())
        levels += len(lv) + 1
    out = (0.5 * bc, reached, edges, levels, K)
    return out + (all32,) if details else out


def within_bound(got, want, K):
    """The largest |got - want| / (gamma(K) want) over the vertices with want > 0 (0 when there is
    none); asserts that got is +0 wherever want is 0 and finite everywhere."""
    got = np.asarray(got)
    g64 = got.astype(np.float64)
    assert np.isfinite(g64).all()
    zero = want == 0
    assert (g64[zero] == 0).all() and not np.signbit(got[zero]).any(), "a vertex off every path is not +0"
    assert (K[~zero] >= 1).all()
    if zero.all():
        return 0.0
    return float((np.abs(g64 - want)[~zero] / (gamma(K[~zero]) * want[~zero])).max())


# ---------------------------------------------------------------------------
# float32 Brandes in the kernel's arithmetic, where the order of the additions cannot matter
# ---------------------------------------------------------------------------
def _low_bit(x):
    """The value of the lowest set mantissa bit of each (positive float32) x."""
    m, e = np.frexp(x)
    M = np.round(m * 2.0 ** 24).astype(np.int64)
    return np.ldexp((M & -M).astype(np.float64), e - 24)


def _row_sums(rows, terms, n):
    """(sums, touched, order_free).  A row's sum is the same in every order when all its terms are
    multiples of one power of two q and the total is at most 2^24 q: then every partial sum of every
    subset is such a multiple too, hence a float32 value, and no addition rounds."""
    tot = np.zeros(n)
    np.add.at(tot, rows, terms)
    q = np.full(n, np.inf)
    np.minimum.at(q, rows, _low_bit(terms))
    touched = np.isfinite(q)
    free = bool((tot[touched] <= 2.0 ** 24 * q[touched]).all() and (tot[touched] <= FLT_MAX).all())
    return tot, touched, free


def bc_order_free(ap, aj, sources):
    """(bc as float32, free).  When `free`, bc is what ANY correct float32 evaluation of the
    kernel's formulas returns, bit for bit: every sum is order-free (_row_sums), every product
    sigma * sum is exact (so fma(sigma, sum, 1) == fl(1 + delta)), each quotient is rounded once,
    correctly, and bc += 0.5 * delta is rounded once per source in source order."""
    G = LevelGraph(ap, aj)
    n = G.n
    f32 = np.float32
    bc = np.zeros(n, f32)
    free = True
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        for s in sources:
            depth, lv = G.search(int(s))
            sigma = np.zeros(n)
            sigma[s] = 1.0
            for u, w in lv:
                tot, touched, ok = _row_sums(w, sigma[u], n)
                free = free and ok
                sigma = np.where(touched, tot, sigma)
            sigma32 = sigma.astype(f32)
            rho32 = np.where(depth >= 0, f32(1) / sigma32, f32(0)).astype(f32)
            free = free and bool((rho32[depth >= 0] >= np.finfo(f32).tiny).all())  # normal reciprocals only
            for u, w in lv[:0:-1]:  # level 0 is the source: no delta
                tot, touched, ok = _row_sums(u, rho32[w].astype(np.float64), n)
                delta = sigma * tot  # exact in float64: 24 x 24 bits
                free = free and ok and _is_float32(delta[touched])
                delta32 = delta.astype(f32)
                rho32 = np.where(touched, (f32(1) + delta32) / sigma32, rho32).astype(f32)
                free = free and bool((rho32[touched] >= np.finfo(f32).tiny).all())
                bc = np.where(touched, bc + f32(0.5) * delta32, bc).astype(f32)
    return bc, free


# ---------------------------------------------------------------------------
# builders: (ap, aj, ids).  Undirected unless directed=True, when every edge points away from the
# first vertex named; `dup` parallel copies of an edge are `dup` separate paths.
# ---------------------------------------------------------------------------
def _build(n, edges, directed, ids):
    ap, aj = csr(n, edges, symmetric=not directed)
    return ap, aj, ids


def _pairs(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.int64), np.asarray(b, np.int64))
    return np.stack([a.ravel(), b.ravel()], 1)


def star(m, directed=False, dup=1):
    """hub 0 and m leaves."""
    leaves = np.arange(1, m + 1)
    return _build(m + 1, np.repeat(_pairs(0, leaves), dup, 0), directed, {"hub": 0, "leaves": leaves})


def out_fan(m, directed=False, dup=1):
    """s - h - m leaves: h has one edge in and m out."""
    leaves = np.arange(2, m + 2)
    edges = np.concatenate([_pairs(0, 1), _pairs(1, leaves)])
    return _build(m + 2, np.repeat(edges, dup, 0), directed, {"s": 0, "h": 1, "leaves": leaves})


def fan_in(m, directed=False, dup=1):
    """s - A(m) - h: h has m edges in and none out."""
    A = np.arange(1, m + 1)
    edges = np.concatenate([_pairs(0, A), _pairs(A, m + 1)])
    return _build(m + 2, np.repeat(edges, dup, 0), directed, {"s": 0, "A": A, "h": m + 1})


def funnel(m1, m2, tail=True, dup=1, directed=False):
    """s - A(m1) - h - B(m2) [- t], with `dup` parallel copies of each s - a edge."""
    A = np.arange(1, m1 + 1)
    h = m1 + 1
    B = np.arange(m1 + 2, m1 + m2 + 2)
    t = m1 + m2 + 2
    edges = [np.repeat(_pairs(0, A), dup, 0), _pairs(A, h), _pairs(h, B)]
    if tail:
        edges.append(_pairs(B, t))
    ids = {"s": 0, "A": A, "h": h, "B": B}
    if tail:
        ids["t"] = t
    return _build(t + 1 if tail else t, np.concatenate(edges), directed, ids)


def diamonds(k, directed=False):
    """A chain of k diamonds c_i - {x_i, y_i} - c_{i+1}, c_i = 3 i: 2^k shortest paths end to end."""
    c = 3 * np.arange(k)
    edges = np.concatenate([_pairs(c, c + 1), _pairs(c, c + 2), _pairs(c + 1, c + 3), _pairs(c + 2, c + 3)])
    return _build(3 * k + 1, edges, directed, {"c": np.append(c, 3 * k)})


def bipartite_layer(a, b, directed=False):
    """s - A(a), and A x B(b) complete."""
    A = np.arange(1, a + 1)
    B = np.arange(a + 1, a + b + 1)
    edges = np.concatenate([_pairs(0, A), _pairs(A[:, None], B[None, :])])
    return _build(a + b + 1, edges, directed, {"s": 0, "A": A, "B": B})


# ---------------------------------------------------------------------------
# the cases the device is held to bit for bit: name -> () -> (ap, aj, sources, symmetric).
# tests/test_bc_oracle.py asserts that each of them is order-free.
# ---------------------------------------------------------------------------
def _case(builder, pick, *args, **kw):
    def make():
        ap, aj, ids = builder(*args, **kw)
        return ap, aj, [int(x) for x in pick(ids)], not kw.get("directed", False)
    return make


def bit_cases():
    cases = {}
    for m in BOUNDARY_LENGTHS:
        # the backward hub sum (and, from a leaf, the forward one over unit terms)
        cases[f"star{m}"] = _case(star, lambda i: [i["hub"], i["leaves"][0], i["leaves"][-1]], m)
        cases[f"star{m}_directed"] = _case(star, lambda i: [i["hub"]], m, directed=True)
        # in = 1, out = m
        cases[f"out_fan{m}_directed"] = _case(out_fan, lambda i: [i["s"]], m, directed=True)
        cases[f"out_fan{m}"] = _case(out_fan, lambda i: [i["s"], i["h"], i["leaves"][1]], m)
        # the forward hub sum over sigma (not the unit first level), out = 0 when directed
        cases[f"fan_in{m}_directed"] = _case(fan_in, lambda i: [i["s"]], m, directed=True)
        cases[f"fan_in{m}"] = _case(fan_in, lambda i: [i["s"]], m)
        cases[f"fan_in{m}_a_h"] = _case(fan_in, lambda i: [i["A"][0], i["h"]], m)
    s_only = lambda i: [i["s"]]
    # slots sized by the longer direction: the shorter row ends inside the first slot
    cases["funnel4096_2_directed"] = _case(funnel, s_only, 4096, 2, directed=True)
    cases["funnel4096_4_directed"] = _case(funnel, s_only, 4096, 4, directed=True)
    cases["funnel2_4096_notail_directed"] = _case(funnel, s_only, 2, 4096, tail=False, directed=True)
    cases["funnel4_2049_notail_directed"] = _case(funnel, s_only, 4, 2049, tail=False, directed=True)
    cases["funnel256_2048_directed"] = _case(funnel, s_only, 256, 2048, directed=True)
    cases["funnel256_2048_s_t"] = _case(funnel, lambda i: [i["s"], i["t"]], 256, 2048)
    cases["funnel256_2048_a_h_b"] = _case(funnel, lambda i: [i["A"][0], i["h"], i["B"][0]], 256, 2048)
    # parallel edges into hub rows
    for m1, m2 in ((512, 16), (16, 512), (256, 256)):
        for dup in (1, 2):
            cases[f"funnel{m1}_{m2}_dup{dup}_directed"] = _case(funnel, s_only, m1, m2, dup=dup, directed=True)
            cases[f"funnel{m1}_{m2}_dup{dup}"] = _case(funnel, lambda i: [i["s"], i["t"]], m1, m2, dup=dup)
    # path counts far from 1: sigma up to 2^100, rho down to 2^-100, every delta an integer
    cases["diamonds100"] = _case(diamonds, lambda i: [i["c"][0], i["c"][50], i["c"][100]], 100)
    cases["diamonds100_directed"] = _case(diamonds, lambda i: [i["c"][0]], 100, directed=True)
    return cases


def wide_level_case(cus, directed=False):
    """out_fan with more leaves than one trip of bc_level_kernel has lane groups (16 per workgroup,
    8 workgroups per CU): (ap, aj, sources, rows of the widest level, lane groups of a trip)."""
    groups = 16 * 8 * cus
    m = groups + groups // 4 - 960 * cus // 256
    ap, aj, ids = out_fan(m, directed=directed)
    return ap, aj, [ids["s"], int(ids["leaves"][1])], m, groups


def many_slots_case(cus, directed=False):
    """bipartite_layer(256, b) with more hub rows on one level than bc_hub_chunk_kernel's grid has
    workgroups (8 per CU): (ap, aj, sources, chunk slots of that level, workgroups)."""
    grid = 8 * cus
    b = grid + 52
    ap, aj, ids = bipartite_layer(256, b, directed=directed)
    return ap, aj, [ids["s"]], b * chunks_of(256, 0 if directed else 256), grid
