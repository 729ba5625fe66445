"""The PageRank checker (tests/pr_oracle.py) checked on the CPU before it judges the device: a float32
run with the adds in any order stays within HALF of what `reference` allows, and every deliberate
defect -- each a small one that a 5e-6 absolute tolerance cannot see -- puts at least one vertex beyond
FOUR times it.  The second is a condition on the inputs (the builders' weights and `rich` positions),
not a figure measured on the device."""
import numpy as np
import pytest

import pr_oracle as po

ALPHA = 0.85
TS = (1, 3, 10)
CASES = po.cases()
DRAWS = 3            # summation orders per defect: the defect must show under each


def worst(case, T, rng, fault=None):
    ap, aj, aw = case
    p, allowed = po.reference(ap, aj, aw, ALPHA, T)
    return po.ratio(po.emulate(ap, aj, aw, ALPHA, T, rng, fault), p, allowed)


def decisive(case, fault, at=None, seed=7):
    """Smallest over T and DRAWS orders of the largest ratio (over the vertices `at`, default all)."""
    rng = np.random.default_rng(seed)
    least = np.inf
    for T in TS:
        for _ in range(DRAWS):
            r = worst(case, T, rng, fault)
            least = min(least, float((r if at is None else r[np.asarray(at)]).max()))
    return least


# ---------------------------------------------------------------------------
# the graphs are what they claim to be
# ---------------------------------------------------------------------------
def test_builders_are_deterministic_and_well_formed():
    again = po.cases()
    for name, (ap, aj, aw) in CASES.items():
        assert ap.dtype == np.int32 and aj.dtype == np.int32 and aw.dtype == np.float32, name
        assert ap[0] == 0 and ap[-1] == len(aj) == len(aw) and (np.diff(ap) >= 0).all(), name
        assert len(aj) == 0 or (0 <= aj.min() and aj.max() < len(ap) - 1), name
        assert ((aw >= 0) & (aw <= 64) & (aw == np.round(aw))).all(), name
        assert all((x == y).all() for x, y in zip(CASES[name], again[name])), name
        assert len(ap) - 1 <= 8192 and len(aj) <= 70000, name


@pytest.mark.parametrize("m", po.HUB_SIZES)
def test_hub_layout(m):
    ap, aj, aw = po.hub(m)
    tp, edge = po.in_rows(ap, aj)
    src = np.repeat(np.arange(len(ap) - 1), np.diff(ap))
    assert tp[1] - tp[0] == m and tp[2] - tp[1] == m + 3          # in-degrees of the two hubs
    row0 = edge[tp[0]:tp[1]]
    assert (src[row0] == 2 + np.arange(m)).all()                   # leaf j at position j of hub 0's row
    assert [po.hub_edge(ap, aj, j) for j in range(m)] == row0.tolist()
    rich = po.hub_rich(m)
    assert (aw[row0[rich]] == 64).all() and m - 1 in rich and 0 in rich
    rest = np.setdiff1d(np.arange(m), rich)
    assert sorted(set(aw[row0[rest]].tolist())) == [0.0, 1.0] and (aw[row0[rest]] == 0).sum() == 3
    row1 = edge[tp[1]:tp[2]]
    first_zero = int(np.flatnonzero(aw[row0] == 0)[0])
    assert (src[row1[:first_zero]] == 2 + np.arange(first_zero)).all()
    tot = np.bincount(src, weights=aw, minlength=len(ap) - 1)
    assert (tot[2:m + 2] == 65).all() and tot[m + 2] == 0 and np.diff(ap)[m + 2] == 0
    assert po.in_degrees(ap, aj)[m + 2] == 0                       # the isolated vertex
    assert np.diff(ap)[0] == np.diff(ap)[1] == 1                   # one feedback edge per hub
    assert set(aj[:2] - 2) <= set(np.flatnonzero(aw[row0] == 0).tolist()) and not set(aj[:2] - 2) & set(rich)


def test_short_rows_layout():
    ap, aj, aw = po.short_rows()
    k = len(po.SHORT_DEGREES)
    n = len(ap) - 1
    assert po.in_degrees(ap, aj)[:k].tolist() == list(po.SHORT_DEGREES)
    assert sorted(np.diff(ap)[:k].tolist()) == sorted(po.SHORT_DEGREES)
    assert n & (n - 1) != 0
    src = np.repeat(np.arange(n), np.diff(ap))
    assert len(set(zip(src.tolist(), aj.tolist()))) == len(aj)     # no parallel edges here


def test_runs_layout():
    ap, aj, aw = po.runs()
    indeg, tested = po.runs_layout()
    n = len(ap) - 1
    assert po.in_degrees(ap, aj).tolist() == indeg + [0] * (n - len(indeg))
    assert len(aj) % 256 != 0
    tp, _ = po.in_rows(ap, aj)
    seen = set()
    for v, start, length in tested:
        assert tp[v] == start and tp[v + 1] - tp[v] == length
        seen.add((start % 64, length))
    assert seen == {(o, l) for o in po.RUN_OFFSETS for l in po.RUN_LENGTHS}
    crosses = lambda at: any(s % at + l > at for _, s, l in tested)
    assert crosses(64) and crosses(256)


def test_dangling_layout():
    ap, aj, aw = po.dangling()
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap))
    assert n == 1000 and (np.diff(ap) == 0).sum() == 334
    assert np.diff(ap)[1] == 5 and (aw[ap[1]:ap[2]] == 0).all() and po.in_degrees(ap, aj)[1] >= 12
    assert ((src == 2) & (aj == 2)).sum() == 1 and ((src == 4) & (aj == 5)).sum() == 2


# ---------------------------------------------------------------------------
# a correct float32 run stays within half of the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_float32_in_any_order_stays_within_half(name):
    rng = np.random.default_rng(2026)
    top = 0.0
    for T in TS:
        for _ in range(20):
            r = worst(CASES[name], T, rng)
            v = int(np.argmax(r))
            assert r[v] <= 0.5, (name, T, v, float(r[v]))
            top = max(top, float(r[v]))
    print(f"{name}: largest |got - p| / allowed over 60 runs {top:.3f}")


def test_reference_refuses_what_the_bound_does_not_cover():
    ap, aj, aw = po.tiny(3)
    bad = aw.copy()
    bad[1] = -1.0
    with pytest.raises(AssertionError):
        po.reference(ap, aj, bad, ALPHA, 3)
    ap, aj, aw = po.hub(4097)
    with pytest.raises(AssertionError):                            # indeg * u * T >= 1e-2
        po.reference(ap, aj, aw, ALPHA, 50)


# ---------------------------------------------------------------------------
# every defect is seen: some vertex beyond 4 x allowed, whatever the order of the adds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["drop", "twice"])
@pytest.mark.parametrize("m", [256, 257, 2048, 2049, 4097])
def test_one_edge_of_a_hub_row_lost_or_doubled(m, kind):
    case = po.hub(m)
    ap, aj, _ = case
    positions = po.hub_rich(m)
    if m <= 257:
        # an arbitrary light edge: 1/m of the row against m * u.  Among the equal light terms of the
        # larger rows (1/m close to m * u) one edge is NOT decisive, hence `rich`.
        positions = positions + [100]
    for j in positions:
        got = decisive(case, (kind, [po.hub_edge(ap, aj, j)]), at=[0])
        assert got > 4, (m, kind, j, got)


@pytest.mark.parametrize("kind", ["drop", "twice"])
def test_last_edge_of_every_short_row_lost_or_doubled(kind):
    case = po.short_rows()
    ap, aj, _ = case
    tp, edge = po.in_rows(ap, aj)
    rows = [i for i, d in enumerate(po.SHORT_DEGREES) if d]
    fault = (kind, [int(edge[tp[i + 1] - 1]) for i in rows])
    for i in rows:                                                 # decisive at EVERY one of the rows
        got = decisive(case, fault, at=[i])
        assert got > 4, (kind, po.SHORT_DEGREES[i], got)


@pytest.mark.parametrize("kind", ["drop", "twice"])
@pytest.mark.parametrize("end", ["first", "last"])
def test_end_of_every_run_lost_or_doubled(kind, end):
    case = po.runs()
    ap, aj, _ = case
    tp, edge = po.in_rows(ap, aj)
    _, tested = po.runs_layout()
    fault = (kind, [int(edge[tp[v]] if end == "first" else edge[tp[v + 1] - 1]) for v, _, _ in tested])
    for v, start, length in tested:
        got = decisive(case, fault, at=[v])
        assert got > 4, (kind, end, start % 64, length, got)


@pytest.mark.parametrize("name", ["short_rows", "runs", "dangling", "random", "hub257", "hub2049", "tiny3"])
def test_transpose_confused(name):
    assert decisive(CASES[name], ("transpose",)) > 4, name


def test_dangling_mass():
    case = po.dangling()
    assert decisive(case, ("no_dangling",)) > 4
    assert decisive(case, ("zero_row_live",)) > 4
    # the isolated vertex and the hubs' target-less leaves are the dangling mass of hub(m), too
    assert decisive(po.hub(257), ("no_dangling",)) > 4


def test_ranks_delivered_in_the_wrong_numbering():
    case = po.random_directed()
    frm = po.degree_sorted(case[0])
    assert (frm[frm] != np.arange(len(frm))).any()                 # no involution: scatter != gather
    assert decisive(case, ("scatter", frm)) > 4
    # two low-degree vertices swapped, everything else in place
    swap = np.arange(len(frm))
    low = np.argsort(np.diff(case[0]), kind="stable")[:2]
    cyc = np.concatenate([low, [int(np.argmax(np.diff(case[0])))]])
    swap[cyc] = np.roll(cyc, 1)                                    # a 3-cycle through them
    assert decisive(case, ("scatter", swap)) > 4


@pytest.mark.parametrize("name", ["random", "dangling", "short_rows", "hub256", "hub4097", "tiny3"])
def test_one_iteration_more_or_less(name):
    # not on runs(): all of its edges end in 45 vertices, which mix so fast that iterations 9, 10 and 11
    # agree to the last bit -- there one iteration more or less is no defect at T = 10
    for d in (-1, 1):
        assert decisive(CASES[name], ("iterations", d)) > 4, (name, d)


@pytest.mark.parametrize("name,block", [("random", 0), ("random", 17), ("random", 31), ("runs", 5),
                                        ("hub4097", 9)])
def test_current_rank_read_for_previous(name, block):
    assert 256 * block < len(CASES[name][1])
    assert decisive(CASES[name], ("stale", block)) > 4, (name, block)
