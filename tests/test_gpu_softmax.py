"""grx_edge_softmax (per-entry scores normalised over a row's or a column's entries: the maximum, the sum of
expf(s - max) in grx_spmv's order, a rounded division) and grx_edge_softmax_backward against numpy: bit
for bit wherever the header's arithmetic fixes the bits (equal scores, masks, NaN, shifted scores, groups on
their own, the backward pass on inputs that tell orders apart), within the derived bound of
softmax_oracle.forward_bound on general scores, and as a differentiable function under autograd.  Every
call is made twice, into nnz floats inside a storage filled with -7 and then NaN, and must repeat itself
and leave the guards alone.  Each case is named for what can go wrong at its shape."""
import os

import numpy as np
import pytest

from softmax_oracle import (backward, backward_in_order, csr, edge_softmax, forward_bound, groups, order_inputs,
                            transpose)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4096]  # test_gpu_sddmm.py's: around a chunk of entries,
                                                             # the minimum segment and the default one
COLUMNS = 4096
SEGMENTS = [None, "64"]
GUARD = 3
INVALID, UNSUPPORTED = -1, -3  # GRX_ERR_INVALID_ARGUMENT, GRX_ERR_UNSUPPORTED
INF, NAN = np.float32(np.inf), np.float32(np.nan)


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def on_device(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def twice(call, g, *inputs, by="row"):
    """Two calls of call(*inputs, by=, out=) into the middle of storages filled with something else: the
    second repeats the first bit for bit and neither touches the guards.  -> (out as numpy, Stats)."""
    import torch
    first = None
    for fill in (-7.0, float("nan")):
        storage = torch.full((g.nnz + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
        out, st = call(*inputs, by=by, out=storage[GUARD:GUARD + g.nnz])
        assert out.data_ptr() == storage.data_ptr() + 4 * GUARD and out.shape == (g.nnz,)
        assert st.iterations == 1 and st.edges_traversed == st.edges_expanded == g.nnz
        assert st.elapsed_ms > 0
        guards = torch.cat([storage[:GUARD], storage[GUARD + g.nnz:]])
        assert bool(torch.isnan(guards).all() if fill != fill else (guards == fill).all()), "a guard was written"
        result = out.cpu().numpy()
        if first is None:
            first = (result, st)
        else:
            assert same_bits(result, first[0])
            assert st.advance_launches == first[1].advance_launches
    return first


def forward(ea, ctx, g, s, by="row"):
    return twice(lambda x, by, out: ea.edge_softmax(ctx, g, x, by=by, out=out), g, on_device(s), by=by)


def back(ea, ctx, g, a, t, by="row"):
    return twice(lambda x, y, by, out: ea.edge_softmax_backward(ctx, g, x, y, by=by, out=out), g, on_device(a),
                 on_device(t), by=by)


def hook(monkeypatch, segment):
    if segment:
        monkeypatch.setenv("GRX_SOFTMAX_SEGMENT", segment)


@pytest.fixture(scope="module")
def rmat(ea, ctx):
    """2**10 vertices, symmetric: more than one sweep of a workgroup, empty rows, and hub rows that the
    hook at its minimum cuts into many items and the default into a few."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7)
    ap, aj, _ = g.to_host()
    degree = np.diff(ap)
    assert degree.max() > 512 and (degree == 0).any()
    return g, ap, aj


@pytest.fixture(scope="module")
def directed(ea, ctx):
    """The directed R-MAT of the same size with its in-edges, and the same structure without them."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    in_degree = np.diff(transpose(ap, aj, aw)[0])
    assert in_degree.max() > 64 and (in_degree == 0).any()  # a column that the hook at its minimum cuts
    return g, ap, aj, ea.Graph.from_host_csr(ap, aj, aw)


@pytest.fixture(scope="module")
def ladder(ea):
    rng = np.random.default_rng(11)
    ap = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.int32)
    aj = np.concatenate([rng.permutation(COLUMNS)[:d] for d in LADDER]).astype(np.int32)  # rows not sorted
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols=COLUMNS), ap, aj


CASES = [("rmat", "row"), ("ladder", "row"), ("directed", "column")]


@pytest.fixture
def graphs(rmat, ladder, directed):
    return {"rmat": rmat, "ladder": ladder, "directed": directed[:3]}


def group_of(ap, aj, by):
    """-> (list of position arrays, per entry the index of its group)."""
    gs = groups(ap, aj, by)
    owner = np.zeros(len(aj), np.int64)
    for i, at in enumerate(gs):
        owner[at] = i
    return gs, owner


# ---- exact forward -------------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("name,by", CASES)
def test_equal_scores_give_one_nth(ea, ctx, graphs, monkeypatch, name, by, segment):
    """Every score of a group is one per-group constant, 1e30, -1e30 and 0 among them: s - m is 0, every
    term is 1, sums of ones are exact in any order, and the division rounds once."""
    g, ap, aj = graphs[name]
    gs, owner = group_of(ap, aj, by)
    rng = np.random.default_rng(2)
    constant = rng.choice(np.array([1e30, -1e30, 0.0, -3.5, 88.0, 1e-30], np.float32), len(gs))
    hook(monkeypatch, segment)
    out, st = forward(ea, ctx, g, constant[owner], by)
    size = np.array([len(at) for at in gs], np.float32)
    assert same_bits(out, (np.float32(1) / size[owner]).astype(np.float32))
    assert st.advance_launches == 6  # the plan, the short groups, and four kernels for the long ones


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("name,by", CASES)
def test_masks_and_poisoned_groups(ea, ctx, graphs, monkeypatch, name, by, segment):
    """Scores in {c, -inf} give 1 / count(c) and exact zeros; a fully masked group gives zeros; a group
    with a NaN, a +inf, or a NaN beside nothing but -inf is NaN throughout -- and the bits of every
    other group are what they are without the poison."""
    g, ap, aj = graphs[name]
    gs, owner = group_of(ap, aj, by)
    rng = np.random.default_rng(3)
    constant = rng.choice(np.array([1e30, -1e30, 0.0, 7.25], np.float32), len(gs))
    s = constant[owner].copy()
    s[rng.random(len(s)) < 0.4] = -INF
    sizes = np.array([len(at) for at in gs])
    largest = int(sizes.argmax())
    full = sorted({i for i in range(len(gs)) if sizes[i] and i % 5 == 0} | {largest})  # fully masked ones
    for i in full:
        s[gs[i]] = -INF
    hook(monkeypatch, segment)
    clean, _ = forward(ea, ctx, g, s, by)
    want = np.zeros(len(s), np.float32)
    for at in gs:
        kept = at[s[at] != -INF]
        want[kept] = np.float32(1) / np.float32(max(len(kept), 1))
    assert same_bits(clean, want) and not np.signbit(clean).any()
    assert sizes[largest] > 64 and any(0 < sizes[i] <= 64 for i in full)  # long and short ones

    poisoned = s.copy()
    kinds = {}
    chosen = sorted({i for i in range(len(gs)) if sizes[i] and i % 3 == 0} | {largest, int(np.argsort(sizes)[-2])})
    for count, i in enumerate(chosen):
        at = gs[i]
        kind = count % 3
        where = at[rng.integers(len(at))]
        if kind == 0:
            poisoned[where] = NAN
        elif kind == 1:
            poisoned[where] = INF
        else:  # NaN beside -inf alone: the maximum must not skip the NaN
            poisoned[at] = -INF
            poisoned[where] = NAN
        kinds[i] = kind
    assert {0, 1, 2} == set(kinds.values()) and sizes[largest] > 64 and largest in kinds
    out, _ = forward(ea, ctx, g, poisoned, by)
    hit = np.isin(owner, list(kinds))
    assert np.isnan(out[hit]).all() and same_bits(out[~hit], clean[~hit])


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("name,by", CASES)
def test_shift_invariance(ea, ctx, graphs, monkeypatch, name, by, segment):
    """Integer scores in [-20, 0] and the same plus 1000: every s - m is the same exact integer."""
    g, ap, aj = graphs[name]
    s = np.random.default_rng(4).integers(-20, 1, g.nnz).astype(np.float32)
    hook(monkeypatch, segment)
    out, _ = forward(ea, ctx, g, s, by)
    shifted, _ = forward(ea, ctx, g, s + np.float32(1000), by)
    assert same_bits(shifted, out) and len(np.unique(out)) > 20


# ---- a group's bits are its own ------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
def test_every_ladder_row_alone(ea, ctx, ladder, monkeypatch, segment):
    g, ap, aj = ladder
    rng = np.random.default_rng(5)
    s = rng.uniform(-16, 16, g.nnz).astype(np.float32)
    a, t = order_inputs(rng, g.nnz)
    hook(monkeypatch, segment)
    out, _ = forward(ea, ctx, g, s)
    grad, _ = back(ea, ctx, g, a, t)
    for r, d in enumerate(LADDER):
        if d == 0:
            continue
        lo, hi = ap[r], ap[r + 1]
        alone = ea.Graph.from_host_csr(np.array([0, d], np.int32), aj[lo:hi], np.ones(d, np.float32), n_cols=COLUMNS)
        assert same_bits(forward(ea, ctx, alone, s[lo:hi])[0], out[lo:hi]), d
        assert same_bits(back(ea, ctx, alone, a[lo:hi], t[lo:hi])[0], grad[lo:hi]), d


@pytest.mark.parametrize("segment", SEGMENTS)
def test_a_column_alone(ea, ctx, directed, monkeypatch, segment):
    """The longest column of the directed graph and a short one, each as the only column of a graph with
    the same rows: the entries keep their rows, so their order in the column is the same."""
    g, ap, aj, _ = directed
    gs, _ = group_of(ap, aj, "column")
    rng = np.random.default_rng(6)
    s = rng.uniform(-16, 16, g.nnz).astype(np.float32)
    hook(monkeypatch, segment)
    out, _ = forward(ea, ctx, g, s, "column")
    sizes = np.array([len(at) for at in gs])
    for c in (int(sizes.argmax()), int(np.flatnonzero((sizes > 1) & (sizes <= 16))[0])):
        at = gs[c]
        row = np.searchsorted(ap, at, side="right") - 1
        one_ap, one_aj, _ = csr(g.n_rows, np.stack([row, np.full(len(at), c)], axis=1), symmetric=False)
        alone = ea.Graph.from_host_csr(one_ap, one_aj, np.ones(len(at), np.float32)).build_in_edges(ctx)
        assert same_bits(forward(ea, ctx, alone, s[at], "column")[0], out[at]), c
    assert sizes.max() > 64


@pytest.mark.parametrize("segment", SEGMENTS)
def test_by_column_on_a_symmetric_graph_is_by_row_at_the_mirror(ea, ctx, monkeypatch, segment):
    """The symmetric R-MAT with one entry per pair and sorted rows, so that every entry (r, c) has one
    mirror (c, r): with mirror-equal scores column c's entries, in ascending position, carry the scores
    of row c's entries in row order."""
    ap, aj, _ = ea.Graph.rmat(ctx, 10, 16, 1, 7).to_host()
    n = len(ap) - 1
    key = np.unique(np.repeat(np.arange(n, dtype=np.int64), np.diff(ap)) * (n + 1) + aj)
    row, col = key // (n + 1), key % (n + 1)
    ap = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int32)
    g = ea.Graph.from_host_csr(ap, col.astype(np.int32), np.ones(len(col), np.float32)).build_in_edges(ctx)
    mirror = np.searchsorted(key, col * len(ap) + row)
    assert (key[mirror] == col * len(ap) + row).all()
    rng = np.random.default_rng(7)
    pair = rng.uniform(-16, 16, (len(ap), len(ap))).astype(np.float32)
    s = np.where(row < col, pair[row, col], pair[col, row]).astype(np.float32)
    assert same_bits(s[mirror], s) and np.diff(ap).max() > 64
    hook(monkeypatch, segment)
    by_row, _ = forward(ea, ctx, g, s)
    by_column, _ = forward(ea, ctx, g, s, "column")
    assert same_bits(by_column, by_row[mirror]) and not same_bits(by_column, by_row)


# ---- general scores ------------------------------------------------------------------------------------

def general_scores(rng, gs, nnz):
    """Scores of spread at most 32 within a group, around per-group centres far apart."""
    s = np.zeros(nnz, np.float32)
    for at in gs:
        s[at] = np.float32(rng.uniform(-1000, 1000)) + rng.uniform(-15.9, 15.9, len(at)).astype(np.float32)
    return s


def within_the_bound(out, s, ap, aj, by):
    gs = groups(ap, aj, by)
    want = edge_softmax(ap, aj, s, by)
    worst = 0.0
    for at in gs:
        if len(at) == 0:
            continue
        spread = float(s[at].max()) - float(s[at].min())
        assert spread <= 32.0
        bound = forward_bound(len(at), spread)
        error = np.abs(out[at].astype(np.float64) - want[at]) / want[at]
        worst = max(worst, float(error.max() / bound))
        assert (error <= bound).all(), (len(at), float(error.max()), bound)
        assert abs(out[at].astype(np.float64).sum() - 1.0) <= len(at) * 2.0 ** -23
    print(f"worst error / bound: {worst:.3f}")


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("name,by", [("rmat", "row"), ("directed", "column")])
def test_general_scores_within_the_bound(ea, ctx, graphs, monkeypatch, name, by, segment):
    """Every entry, none left out, against float64 within forward_bound for its group's length and
    spread, and every non-empty group sums to 1 within n * 2**-23."""
    g, ap, aj = graphs[name]
    s = general_scores(np.random.default_rng(8), groups(ap, aj, by), g.nnz)
    hook(monkeypatch, segment)
    out, _ = forward(ea, ctx, g, s, by)
    within_the_bound(out, s, ap, aj, by)


def test_chesapeake_within_the_bound(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    s = general_scores(np.random.default_rng(9), groups(ap, aj, "row"), g.nnz)
    out, st = forward(ea, ctx, g, s)
    within_the_bound(out, s, ap, aj, "row")
    assert st.advance_launches == 1


# ---- backward ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("name,by", CASES)
def test_backward_in_the_written_order(ea, ctx, graphs, monkeypatch, name, by, segment):
    """Inputs on which nearly every step rounds (tests/test_softmax_abi.py shows that they tell the lane
    order from a sequential and a reversed sum): every bit is the header's order's.  Then integers,
    which any order gets exactly."""
    g, ap, aj = graphs[name]
    rng = np.random.default_rng(10)
    a, t = order_inputs(rng, g.nnz)
    hook(monkeypatch, segment)
    out, st = back(ea, ctx, g, a, t, by)
    want = backward_in_order(ap, aj, a, t, int(segment or 512), by)
    assert same_bits(out, want), np.argwhere(out.view(np.uint32) != want.view(np.uint32))[:8]
    assert st.advance_launches == 5  # the plan, the short groups, the items' sums, the totals, the results
    a = rng.integers(0, 4, g.nnz).astype(np.float32)
    t = rng.integers(-8, 9, g.nnz).astype(np.float32)
    exact = backward(ap, aj, a, t, by)
    assert (np.abs(exact) < 2 ** 24).all()
    assert (back(ea, ctx, g, a, t, by)[0].astype(np.float64) == exact).all()


# ---- refusals and empty shapes -------------------------------------------------------------------------

def test_refusals(ea, ctx, rmat, ladder, directed):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    assert g.nnz == 6
    all_of_it = torch.ones(18, dtype=torch.float32, device="cuda")
    s, t, out = all_of_it[:6], all_of_it[6:12], all_of_it[12:]
    ps, pt, po = s.data_ptr(), t.data_ptr(), out.data_ptr()

    def refused(rc, name):
        return rc == INVALID and name in lib.grx_last_error()

    def fwd(c, h, a, o, by=0):
        return lib.grx_edge_softmax(c, h, by, a, o, None, None)

    def bwd(c, h, a, b, o, by=0):
        return lib.grx_edge_softmax_backward(c, h, by, a, b, o, None, None)

    f, b = b"grx_edge_softmax", b"grx_edge_softmax_backward"
    assert refused(fwd(None, g._h, ps, po), f) and refused(fwd(ctx._h, None, ps, po), f)
    assert refused(fwd(ctx._h, g._h, None, po), f) and refused(fwd(ctx._h, g._h, ps, None), f)
    assert refused(bwd(None, g._h, ps, pt, po), b) and refused(bwd(ctx._h, None, ps, pt, po), b)
    assert refused(bwd(ctx._h, g._h, None, pt, po), b) and refused(bwd(ctx._h, g._h, ps, None, po), b)
    assert refused(bwd(ctx._h, g._h, ps, pt, None), b)
    for shifted in (ps, all_of_it[5:].data_ptr(), all_of_it[1:].data_ptr()):  # the same; one element in common
        assert refused(fwd(ctx._h, g._h, ps, shifted), f) and b"overlap" in lib.grx_last_error()
    for shifted in (ps, pt, all_of_it[5:].data_ptr(), all_of_it[11:].data_ptr(), all_of_it[3:].data_ptr()):
        assert refused(bwd(ctx._h, g._h, ps, pt, shifted), b) and b"overlap" in lib.grx_last_error()
    ctx.synchronize()
    assert (all_of_it == 1).all()  # nothing was launched
    assert fwd(ctx._h, g._h, ps, po) == 0 and bwd(ctx._h, g._h, ps, ps, all_of_it[6:12].data_ptr()) == 0
    ctx.synchronize()  # side by side is fine, and the inputs of the backward call may be one array
    assert out.tolist() == [1.0, 0.5, 0.5, 0.5, 0.5, 1.0] and t.tolist() == [0.0, -1.0, -1.0, -1.0, -1.0, 0.0]

    # by column: without in-edges, on a symmetric handle too, and on a rectangular one
    def unsupported(call):
        with pytest.raises(ea.EngineError) as e:
            call()
        message = lib.grx_last_error()
        return e.value.code == UNSUPPORTED and b"grx_edge_softmax" in message, message

    for handle in (g, rmat[0], directed[3]):
        x = torch.zeros(handle.nnz, dtype=torch.float32, device="cuda")
        ok, message = unsupported(lambda: ea.edge_softmax(ctx, handle, x, by="column"))
        assert ok and b"grx_graph_build_in_edges" in message
        ok, message = unsupported(lambda: ea.edge_softmax_backward(ctx, handle, x, x, by="column"))
        assert ok and b"grx_edge_softmax_backward" in message and b"grx_graph_build_in_edges" in message
    wide = ladder[0]
    x = torch.zeros(wide.nnz, dtype=torch.float32, device="cuda")
    assert unsupported(lambda: ea.edge_softmax(ctx, wide, x, by="column"))[0]
    assert unsupported(lambda: ea.edge_softmax_backward(ctx, wide, x, x, by="column"))[0]

    # the Python layer
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, s, by="rows")
    with pytest.raises(ValueError):
        ea.edge_softmax_backward(ctx, g, s, t, by=0)
    with pytest.raises(ValueError):
        ea.edge_softmax_autograd(ctx, g, s, by="col")
    with pytest.raises(TypeError):
        ea.edge_softmax(ctx, g, s.double())
    with pytest.raises(TypeError):
        ea.edge_softmax(ctx, g, None)
    with pytest.raises(TypeError):
        ea.edge_softmax_backward(ctx, g, s, t.long())
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, all_of_it[:5])                                  # a short vector
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, all_of_it[:12][::2])                            # not contiguous
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, all_of_it[:6].view(2, 3))                       # not a vector
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, s.cpu())
    with pytest.raises(ValueError):
        ea.edge_softmax(ctx, g, s, out=all_of_it[:7])
    with pytest.raises(ValueError):
        ea.edge_softmax_backward(ctx, g, s, t.cpu())
    with pytest.raises(ea.EngineError) as e:
        ea.edge_softmax(ctx, g, s, out=all_of_it[3:9])
    assert e.value.code == INVALID


def test_no_entries_launches_nothing(ea, ctx):
    import torch
    ap, aj, aw = csr(5, [])
    empty = torch.zeros(0, dtype=torch.float32, device="cuda")
    for g in (ea.Graph.from_host_csr(ap, aj, aw), ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])):
        for out, st in (ea.edge_softmax(ctx, g, empty), ea.edge_softmax_backward(ctx, g, empty, empty)):
            assert out.shape == (0,) and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0


def test_groups_within_a_segment_take_fewer_launches(ea, ctx, rmat, monkeypatch):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    s = np.zeros(g.nnz, np.float32)
    small = (forward(ea, ctx, g, s)[1].advance_launches, back(ea, ctx, g, s, s)[1].advance_launches)
    assert small == (1, 1)
    hook(monkeypatch, "64")
    big, ap, aj = rmat
    s = np.zeros(big.nnz, np.float32)
    cut = (forward(ea, ctx, big, s)[1].advance_launches, back(ea, ctx, big, s, s)[1].advance_launches)
    assert cut == (6, 5) and small[0] < cut[0] and small[1] < cut[1]


# ---- autograd ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_directed(ea, ctx):
    g = ea.Graph.rmat(ctx, 8, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    return g.build_in_edges(ctx), ap, aj, ea.Graph.from_host_csr(ap, aj, aw)


def leaf(x, grad=True):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("by", ["row", "column"])
def test_autograd_is_the_two_calls(ea, ctx, small_directed, by):
    """The function's value is edge_softmax's and its gradient is edge_softmax_backward(out, T), bit for
    bit; and the gradient agrees with float64.

    The bound, per entry e of a group of n entries with spread at most 32, u = 2**-24, f =
    forward_bound(n, 32) (the relative error of every a[e]), T in [-1, 1]:
      exact gradient      G = a (T - D),  D = sum a T,  sum a = 1, so |D| <= 1 and |T - D| <= 2;
      D computed from the computed a: every term a T is off by at most f |a T| and rounds once (fused),
        the sum adds at most n - 1 roundings of partial sums that are at most sum |a T| (1 + f) <= 1 + f:
        |dD| <= f + (n + 1) u (1 + f);
      T - D rounds once: |d(T - D)| <= |dD| + 2 u (1 + ...);
      the product rounds once and a is off by f a:
        |dG| <= a (|dD| + 2 u) + f a |T - D| + u |G|  <=  a (f + (n + 3) u + 2 f + 2 u), with 1 % on top:
      |dG| <= 1.01 * a[e] * (3 f + (n + 5) u)."""
    import torch
    g, ap, aj, _ = small_directed
    rng = np.random.default_rng(44)
    gs = groups(ap, aj, by)
    s = general_scores(rng, gs, g.nnz)
    T = rng.uniform(-1, 1, g.nnz).astype(np.float32)
    sd, Td = leaf(s), on_device(T)
    out = ea.edge_softmax_autograd(ctx, g, sd, by=by)
    assert out.requires_grad
    plain, _ = ea.edge_softmax(ctx, g, sd.detach(), by=by)
    assert same_bits(out.detach().cpu().numpy(), plain.cpu().numpy())
    (out * Td).sum().backward()
    want, _ = ea.edge_softmax_backward(ctx, g, plain, Td, by=by)
    grad = sd.grad.cpu().numpy()
    assert same_bits(grad, want.cpu().numpy())

    # float64 on the CPU: the composition that torch differentiates itself
    s64 = torch.from_numpy(s.astype(np.float64)).requires_grad_(True)
    T64 = torch.from_numpy(T.astype(np.float64))
    total = 0
    for at in gs:
        if len(at):
            idx = torch.from_numpy(at)
            total = total + (torch.softmax(s64[idx], dim=0) * T64[idx]).sum()
    total.backward()
    exact = s64.grad.numpy()
    a64 = edge_softmax(ap, aj, s, by)
    worst = 0.0
    for at in gs:
        if len(at) == 0:
            continue
        n = len(at)
        bound = 1.01 * a64[at] * (3 * forward_bound(n, 32.0) + (n + 5) * 2.0 ** -24)
        error = np.abs(grad[at].astype(np.float64) - exact[at])
        worst = max(worst, float((error / bound).max()))
        assert (error <= bound).all(), (n, float((error / bound).max()))
    print(f"worst gradient error / bound: {worst:.3f}")


def test_the_full_layer(ea, ctx, small_directed):
    """sddmm, edge softmax, spmm with values: backward() reaches q, k and x, and on the handle without
    in-edges it raises where spmm's transposed product does."""
    import torch
    g, ap, aj, bare = small_directed
    rng = np.random.default_rng(45)
    F = 6

    def layer(handle):
        q = leaf(rng.standard_normal((g.n_rows, F)) / 2)
        k = leaf(rng.standard_normal((g.n_cols, F)) / 2)
        x = leaf(rng.standard_normal((g.n_cols, F)))
        s = ea.sddmm_autograd(ctx, handle, q, k)
        a = ea.edge_softmax_autograd(ctx, handle, s)
        return q, k, x, a, ea.spmm_autograd(ctx, handle, x, values=a)

    q, k, x, a, h = layer(g)
    sums = torch.zeros(g.n_rows, device="cuda").index_add_(
        0, torch.from_numpy(np.repeat(np.arange(g.n_rows), np.diff(ap))).cuda(), a.detach())
    occupied = torch.from_numpy(np.diff(ap) > 0).cuda()
    assert bool(((sums[occupied] - 1).abs() < 1e-5).all())
    (h * h).sum().backward()
    for leaf_ in (q, k, x):
        assert leaf_.grad is not None and bool(torch.isfinite(leaf_.grad).all()) and bool((leaf_.grad != 0).any())
    q, k, x, a, h = layer(bare)
    with pytest.raises(ea.EngineError):
        h.sum().backward()
