"""The betweenness-centrality checkers (tests/bc_oracle.py) checked on the CPU before they judge the
device: every case the device is held to bit for bit is order-free, the order-free values agree with
the float64 Brandes, a sequential float32 Brandes with its edges in any order keeps to the rounding
bound, and the bound sees one dropped edge of a 300-edge row (and does not see one of a 4096-edge
row, which is why those lengths are tested bit for bit)."""
import os

import numpy as np
import pytest

import bc_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = bo.bit_cases()
f32 = np.float32


def brandes32(ap, aj, sources, rng=None, drop=None):
    """The kernel's formulas in sequential float32: np.add.at adds one edge at a time, in the order
    given -- shuffled per level when `rng` is set.  drop = (u, w): the first such edge is left out
    of the forward sum."""
    G = bo.LevelGraph(ap, aj)
    n = G.n
    bc = np.zeros(n, f32)
    for s in sources:
        depth, lv = G.search(int(s))
        if rng is not None:
            lv = [(u[p], w[p]) for u, w in lv for p in [rng.permutation(len(u))]]
        sigma = np.zeros(n, f32)
        sigma[s] = 1
        for u, w in lv:
            if drop is not None:
                hit = np.flatnonzero((u == drop[0]) & (w == drop[1]))[:1]
                u, w = np.delete(u, hit), np.delete(w, hit)
            np.add.at(sigma, w, sigma[u])
        with np.errstate(divide="ignore"):
            rho = (f32(1) / sigma).astype(f32)
        for u, w in lv[:0:-1]:
            total = np.zeros(n, f32)
            np.add.at(total, u, rho[w])
            touched = np.zeros(n, bool)
            touched[u] = True
            delta = (sigma * total).astype(f32)
            fused = (1.0 + sigma.astype(np.float64) * total.astype(np.float64)).astype(f32)
            with np.errstate(divide="ignore", invalid="ignore"):
                rho = np.where(touched, fused / sigma, rho).astype(f32)
            bc = np.where(touched, bc + f32(0.5) * delta, bc).astype(f32)
    return bc


# ---------------------------------------------------------------------------
# the references on graphs small enough to do by hand
# ---------------------------------------------------------------------------
def test_brandes64_by_hand():
    ap, aj = bo.csr(3, [(0, 1), (1, 2)])
    bc, reached, edges, levels, K = bo.brandes64(ap, aj, range(3))
    assert bc.tolist() == [0.0, 1.0, 0.0] and (reached, edges, levels) == (9, 12, 3 + 2 + 3)
    # two parallel edges are two paths: 0 =2= 1 - 3, 0 - 2 - 3
    ap, aj = bo.csr(4, [(0, 1), (0, 1), (1, 3), (0, 2), (2, 3)], symmetric=False)
    bc, reached, edges, levels, K = bo.brandes64(ap, aj, [0])
    assert np.allclose(bc, [0, 0.5 * 2 / 3, 0.5 / 3, 0]) and (reached, edges, levels) == (4, 5, 3)
    # s -> A(3) -> h: sigma[h] rounds twice, rho[h] once more, delta[a] = 1 * rho[h] once more, bc once more
    ap, aj, ids = bo.fan_in(3, directed=True)
    bc, _, _, _, K = bo.brandes64(ap, aj, [ids["s"]])
    assert K.tolist() == [0, 5, 5, 5, 0] and np.allclose(bc[1:4], 0.5 / 3)
    got, free = bo.bc_order_free(ap, aj, [ids["s"]])
    assert free and (got[1:4] == f32(0.5) * (f32(1) / f32(3))).all() and got[0] == got[4] == 0


def test_builders():
    for directed in (False, True):
        ap, aj, ids = bo.funnel(5, 7, dup=3, directed=directed)
        out, into = np.diff(ap), np.bincount(aj, minlength=len(ap) - 1)
        h, t = ids["h"], ids["t"]
        back = 0 if directed else 1
        assert out[0] == 15 and out[h] == 7 + 5 * back and into[h] == 5 + 7 * back and into[t] == 7
        assert (out[ids["A"]] == 1 + 3 * back).all() and (into[ids["A"]] == 3 + back).all()
        assert len(bo.funnel(5, 7, tail=False, directed=directed)[0]) - 1 == 14
        ap, aj, ids = bo.bipartite_layer(3, 4, directed=directed)
        assert len(aj) == (3 + 12) * (1 + back) and (np.bincount(aj)[ids["B"]] == 3).all()
        ap, aj, ids = bo.diamonds(4, directed=directed)
        assert len(ap) - 1 == 13 and len(aj) == 16 * (1 + back) and ids["c"].tolist() == [0, 3, 6, 9, 12]
        assert bo.brandes64(ap, aj, [0])[3] == 9
    assert [bo.chunks_of(*d) for d in ((255, 3), (3, 256), (2048, 0), (0, 2049), (4097, 4096))] == [0, 1, 1, 2, 3]


# ---------------------------------------------------------------------------
# the bit-for-bit cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BIT))
def test_bit_case_is_order_free_and_agrees_with_float64(name):
    ap, aj, sources, _ = BIT[name]()
    got, free = bo.bc_order_free(ap, aj, sources)
    assert free, name
    want, _, _, _, K, all32 = bo.brandes64(ap, aj, sources, details=True)
    assert bo.within_bound(got, want, K) <= 1.0, name
    if all32:
        assert (got.astype(np.float64) == want).all(), name
    assert (got == brandes32(ap, aj, sources, np.random.default_rng(1))).all(), name


def test_diamonds_up_to_2_126():
    for k in (100, 126):
        for directed, sources in ((False, [0, 3 * (k // 2), 3 * k]), (True, [0])):
            ap, aj, _ = bo.diamonds(k, directed=directed)
            got, free = bo.bc_order_free(ap, aj, sources)
            want, _, _, _, K, all32 = bo.brandes64(ap, aj, sources, details=True)
            assert free and bo.within_bound(got, want, K) <= 1.0, (k, directed)
            assert not directed or (all32 and (got.astype(np.float64) == want).all())
    ap, aj, _ = bo.diamonds(127, directed=True)  # rho = 2^-127 is below the normal range
    assert not bo.bc_order_free(ap, aj, [0])[1]


def test_launch_shape_cases_are_order_free():
    for directed in (False, True):
        ap, aj, sources, slots, grid = bo.many_slots_case(256, directed)
        assert slots == 2100 > grid and 530_000 < len(aj) // (1 if directed else 2) < 550_000
        assert bo.bc_order_free(ap, aj, sources)[1]
    ap, aj, sources, rows, groups = bo.wide_level_case(256)
    assert rows == 40000 and groups < rows < 2 * groups and rows % groups
    assert bo.bc_order_free(ap, aj, sources)[1]


def test_cases_that_are_not_order_free():
    """What must not be compared bit for bit: a quotient with a long mantissa summed over a long row
    (from t, every a of the undirected funnel(4096, 2) hands h the term (1 + 2^-12) / 2)."""
    for args, kw, pick in (((2, 4096), dict(directed=True), "s"), ((4, 4096), dict(directed=True), "s"),
                           ((4096, 2), dict(), "t")):
        ap, aj, ids = bo.funnel(*args, **kw)
        assert not bo.bc_order_free(ap, aj, [ids[pick]])[1], (args, kw)
        want, _, _, _, K = bo.brandes64(ap, aj, [ids[pick]])
        assert bo.within_bound(brandes32(ap, aj, [ids[pick]]), want, K) <= 1.0


# ---------------------------------------------------------------------------
# the bound is sound ...
# ---------------------------------------------------------------------------
def sound(ap, aj, sources, seed):
    want, _, _, _, K = bo.brandes64(ap, aj, sources)
    rng = np.random.default_rng(seed)
    return max(bo.within_bound(brandes32(ap, aj, sources, rng), want, K) for _ in range(3))


FAMILIES = {
    "star300": lambda: (bo.star(300), lambda i: [0, 1, 300]),
    "out_fan2049": lambda: (bo.out_fan(2049), lambda i: [0, 1, 5]),
    "fan_in4097": lambda: (bo.fan_in(4097), lambda i: [0, 1, i["h"]]),
    "funnel255_257": lambda: (bo.funnel(255, 257), lambda i: [0, 7, i["h"], i["t"]]),
    "funnel300_10_directed": lambda: (bo.funnel(300, 10, directed=True), lambda i: [0]),
    "funnel2049_255": lambda: (bo.funnel(2049, 255), lambda i: [0, i["t"], i["B"][3]]),
    "funnel4_4096_directed": lambda: (bo.funnel(4, 4096, directed=True), lambda i: [0]),
    "funnel3_5_dup3": lambda: (bo.funnel(3, 5, dup=3), lambda i: range(11)),
    "diamonds20": lambda: (bo.diamonds(20), lambda i: range(0, 61, 7)),
    "bipartite7_300": lambda: (bo.bipartite_layer(7, 300), lambda i: [0, 3, 100]),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_float32_in_any_edge_order_keeps_to_the_bound(name):
    (ap, aj, ids), pick = FAMILIES[name]()
    top = sound(ap, aj, [int(s) for s in pick(ids)], 2026)
    print(f"{name}: largest error / bound over 3 edge orders {top:.3f}")
    assert top <= 1.0


def test_float32_keeps_to_the_bound_on_chesapeake_and_rmat10(oracle):
    _, ap, aj, _ = oracle.mtx_to_csr(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx"))
    top = sound(ap, np.ascontiguousarray(aj), range(len(ap) - 1), 3)
    print(f"chesapeake, every source: largest error / bound {top:.3f}")
    assert top <= 1.0
    for symmetric in (True, False):
        n, ap, aj, _ = oracle.rmat_csr(10, 16, 1, 7, symmetric)
        aj = np.ascontiguousarray(aj)
        deg = np.diff(ap)
        assert deg.max() >= bo.BC_HUB
        sources = np.random.default_rng(9).choice(np.flatnonzero(deg > 0), 16)
        want, _, _, _, K = bo.brandes64(ap, aj, sources)
        top = sound(ap, aj, sources, 4)
        print(f"rmat10 symmetric={symmetric}: largest error / bound {top:.3f}, largest gamma(K) {bo.gamma(K.max()):.2e}")
        assert top <= 1.0 and bo.gamma(K.max()) < 1e-3


# ---------------------------------------------------------------------------
# ... and not vacuous
# ---------------------------------------------------------------------------
def test_one_dropped_edge_of_a_300_edge_row_breaks_the_bound():
    ap, aj, ids = bo.funnel(300, 10, directed=True)
    want, _, _, _, K = bo.brandes64(ap, aj, [0])
    for a in (ids["A"][0], ids["A"][150], ids["A"][-1]):
        got = brandes32(ap, aj, [0], drop=(a, ids["h"]))
        err = np.abs(got.astype(np.float64) - want)
        allowed = bo.gamma(K) * want
        assert (err[ids["A"]] > 4 * allowed[ids["A"]]).all() and err[ids["h"]] <= allowed[ids["h"]]
    ap, aj, ids = bo.funnel(300, 10)
    want, _, _, _, K = bo.brandes64(ap, aj, [0, ids["t"]])
    got = brandes32(ap, aj, [0, ids["t"]], drop=(ids["A"][299], ids["h"]))
    assert (np.abs(got - want) > 4 * bo.gamma(K) * want)[ids["A"]].all()


def test_one_dropped_edge_of_a_4096_edge_row_is_about_the_bound():
    """gamma(K) of a row of m edges is about m u, one edge of m equal ones is 1 / m: at m = 4096 =
    u^-1/2 the two meet, so these rows are compared bit for bit instead."""
    ap, aj, ids = bo.fan_in(4096, directed=True)
    want, _, _, _, K = bo.brandes64(ap, aj, [0])
    got = brandes32(ap, aj, [0], drop=(ids["A"][7], ids["h"]))
    A = ids["A"]
    ratio = np.abs(got[A] - want[A]) / (bo.gamma(K[A]) * want[A])
    assert 0.5 < ratio.min() and ratio.max() < 2.0
    exact, free = bo.bc_order_free(ap, aj, [0])
    assert free and (got[ids["A"]] != exact[ids["A"]]).all()
