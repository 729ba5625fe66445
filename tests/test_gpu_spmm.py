"""grx_spmm (Y = A X: features on the lanes, a row's entries in row order, long rows cut into segments)
against numpy: bit for bit on integer inputs whose sums float32 holds exactly, bit for bit against the
header's written order on inputs that tell orders apart, within the standard summation bound on general
floats.  Every call is made twice, into outputs filled with -7 and then NaN, and must repeat itself;
what lies between the rows of a strided output must keep the fill.  Each case is named for what can go
wrong at its shape."""
import os

import numpy as np
import pytest

from spmm_oracle import SWEEP_LENGTHS, csr, order_inputs, spmm, spmm_in_order, sweep_ladder, transpose

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4096]  # row lengths around the group of test_gpu_spmv.py,
                                                             # the minimum segment and the default one
COLUMNS = 4096
SEGMENTS = [None, "64"]


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def strided(rows, F, ld, offset, fill):
    """-> (storage, view): a [rows, F] view with row stride ld that begins `offset` floats into a
    storage filled with `fill`."""
    import torch
    storage = torch.full((offset + max(rows, 1) * ld,), fill, dtype=torch.float32, device="cuda")
    return storage, storage[offset:offset + rows * ld].view(rows, ld)[:, :F]


def on_device(x, ld=None, offset=0):
    """The numpy matrix as a device view; what lies between its rows is NaN, so reading it shows."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    _, view = strided(x.shape[0], x.shape[1], ld or x.shape[1], offset, float("nan"))
    view.copy_(torch.from_numpy(x))
    return view


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def twice(ea, ctx, g, xd, transpose=False, ld=None, offset=0):
    """Two calls of ea.spmm into views of storage filled with something else: the second repeats the
    first bit for bit and neither touches what is not an element of y.  -> (y as a numpy array, Stats)
    of the first."""
    import torch
    rows, F = (g.n_cols if transpose else g.n_rows), xd.shape[1]
    first = None
    for fill in (-7.0, float("nan")):
        storage, y = strided(rows, F, ld or F, offset, fill)
        out, st = ea.spmm(ctx, g, xd, transpose=transpose, y=y)
        assert out.data_ptr() == y.data_ptr()
        assert st.iterations == 1 and st.edges_traversed == st.edges_expanded == g.nnz
        assert st.advance_launches >= 1 and st.elapsed_ms > 0
        result = out.cpu().numpy()
        marks, elements = strided(rows, F, ld or F, offset, 0.0)
        elements.fill_(1.0)  # the elements of y within a storage of the same layout
        rest = storage[marks == 0.0]
        assert bool(torch.isnan(rest).all() if fill != fill else (rest == fill).all()), "padding was written"
        if first is None:
            first = (result, st)
        else:
            assert same_bits(result, first[0])
            assert st.advance_launches == first[1].advance_launches
    return first


def integers(rng, shape):
    return rng.integers(0, 16, shape).astype(np.float32)


def exact(y64):
    """An integer product below 2**24 as the float32 it must be."""
    assert (y64 == np.round(y64)).all() and (np.abs(y64) < 2 ** 24).all()
    return y64.astype(np.float32)


@pytest.fixture(scope="module")
def rmat(ea, ctx):
    """2**10 vertices, symmetric: more than one sweep of a workgroup, empty rows, and hub rows that the
    hook at its minimum cuts into many segments and the default into a few."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7)
    ap, aj, aw = g.to_host()
    degree = np.diff(ap)
    assert degree.max() > 512 and degree.max() <= 17000 and (degree == 0).any()
    assert aw.min() >= 1 and aw.max() <= 64 and (aw == np.round(aw)).all()
    return g, ap, aj, aw


@pytest.fixture(scope="module")
def ladder():
    rng = np.random.default_rng(11)
    ap = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.int32)
    aj = np.concatenate([rng.permutation(COLUMNS)[:d] for d in LADDER]).astype(np.int32)  # rows not sorted
    aw = rng.integers(1, 65, len(aj)).astype(np.float32)
    return ap, aj, aw


def hook(monkeypatch, segment):
    if segment:
        monkeypatch.setenv("GRX_SPMM_SEGMENT", segment)


# ---- exact integer products: any order must give these bits -------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [1, 3, 4, 7, 64, 260])
def test_exact_on_a_symmetric_rmat(ea, ctx, rmat, monkeypatch, F, segment):
    """One lane; a tail narrower than a vector; exactly one vector; a vector plus a tail; a quarter
    wavefront per row; more than one 256-wide tile with a ragged last tile."""
    g, ap, aj, aw = rmat
    x = integers(np.random.default_rng(3), (g.n_cols, F))
    hook(monkeypatch, segment)
    y, st = twice(ea, ctx, g, on_device(x))
    assert (y == exact(spmm(ap, aj, aw, x))).all()
    assert st.advance_launches == 4  # the plan, the short rows, the segments, their sums
    # symmetric, no in-edges: the transposed product walks the same rows
    back, _ = twice(ea, ctx, g, on_device(x), transpose=True)
    assert same_bits(back, y)
    if F == 1:
        import torch
        v, _ = ea.spmv(ctx, g, torch.from_numpy(x[:, 0].copy()).cuda())
        assert same_bits(v.cpu().numpy(), y[:, 0])


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [20, 100, 256])
def test_exact_at_the_other_group_widths(ea, ctx, rmat, monkeypatch, F, segment):
    """8 and 32 lanes per row, which the list above does not reach, and a whole wavefront of full vectors."""
    g, ap, aj, aw = rmat
    x = integers(np.random.default_rng(13), (g.n_cols, F))
    hook(monkeypatch, segment)
    y, _ = twice(ea, ctx, g, on_device(x))
    assert (y == exact(spmm(ap, aj, aw, x))).all()


@pytest.mark.parametrize("segment", SEGMENTS)
def test_exact_on_a_rectangular_ladder_through_strided_views(ea, ctx, ladder, monkeypatch, segment):
    """12 rows over 4096 columns: every length at which a chunk of entries or a segment fills up, one
    below and one above.  F = 5 in rows 7 apart (X) and 9 apart (Y): no 16-byte access is possible and
    the two floats (four) between rows are neither read nor written."""
    ap, aj, aw = ladder
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols=COLUMNS)
    assert (g.n_rows, g.n_cols) == (12, COLUMNS)
    x = integers(np.random.default_rng(4), (COLUMNS, 5))
    hook(monkeypatch, segment)
    xd = on_device(x, ld=7)
    assert xd.stride() == (7, 1)
    y, _ = twice(ea, ctx, g, xd, ld=9)
    want = exact(spmm(ap, aj, aw, x))
    assert (y == want).all(), (y, want)
    assert (y[0] == 0).all() and not np.signbit(y[0]).any()


@pytest.mark.parametrize("ld", [8, 10])
def test_views_that_begin_one_float_into_their_storage(ea, ctx, rmat, ld):
    """F = 8 is two full vectors per row, but the base pointer is 4 bytes past a 16-byte boundary (and
    with ld = 10 every other row is 8 past): the call must choose narrower accesses."""
    g, ap, aj, aw = rmat
    x = integers(np.random.default_rng(9), (g.n_cols, 8))
    xd = on_device(x, ld=ld, offset=1)
    assert xd.data_ptr() % 16 == 4 and xd.stride() == (ld, 1)
    y, _ = twice(ea, ctx, g, xd, ld=ld, offset=1)
    assert (y == exact(spmm(ap, aj, aw, x))).all()


@pytest.mark.parametrize("segment", SEGMENTS)
def test_exact_on_the_sweep_ladder(ea, ctx, monkeypatch, segment):
    """37 rows, out-rows forward and in-rows transposed, F = 6: two lanes per row, 32 rows per
    wavefront, so the last wavefront has lane groups past the last row; under the hook a row of 64 is
    short, 65 leaves a segment of one entry and 200 a partial last one."""
    ap, aj, aw = sweep_ladder()
    for offsets in (ap, transpose(ap, aj, aw)[0]):
        assert len(offsets) == 38 and set(SWEEP_LENGTHS) <= set(np.diff(offsets).tolist())
    g = ea.Graph.from_host_csr(ap, aj, aw).build_in_edges(ctx)
    x = integers(np.random.default_rng(8), (37, 6))
    hook(monkeypatch, segment)
    forward, _ = twice(ea, ctx, g, on_device(x))
    back, _ = twice(ea, ctx, g, on_device(x), transpose=True)
    assert (forward == exact(spmm(ap, aj, aw, x))).all()
    assert (back == exact(spmm(ap, aj, aw, x, transpose=True))).all()


# ---- the written order ---------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
def test_the_written_order(ea, ctx, monkeypatch, segment):
    """Features on which nearly every step rounds (tests/test_spmm_abi.py shows that they tell this
    order from its reverse and from grx_spmv's): every bit is the header's order's."""
    lengths = [1, 64, 65, 200, 513, 1025]
    rng = np.random.default_rng(21)
    ap = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    aj = np.concatenate([rng.choice(2048, d, replace=False) for d in lengths]).astype(np.int32)
    aw = rng.integers(1, 65, len(aj)).astype(np.float32)
    x = order_inputs(rng, (2048, 5))
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols=2048)
    hook(monkeypatch, segment)
    y, _ = twice(ea, ctx, g, on_device(x))
    want = spmm_in_order(ap, aj, aw, x, int(segment or 512), order="row")
    assert same_bits(y, want), np.argwhere(y.view(np.uint32) != want.view(np.uint32))


# ---- general floats ------------------------------------------------------------------------------------

def general_graph(ea, ctx, name):
    if name == "chesapeake":
        g = ea.Graph.from_mtx(CHESAPEAKE)
        return (g,) + tuple(g.to_host())
    ap, aj, aw = sweep_ladder()
    return ea.Graph.from_host_csr(ap, aj, aw), ap, aj, aw


@pytest.mark.parametrize("name,segment", [("chesapeake", None), ("sweep_ladder", None), ("sweep_ladder", "64")])
def test_a_column_does_not_notice_the_others(ea, ctx, monkeypatch, name, segment):
    """F = 37 (ten lanes of sixteen at work, a ragged last one) on general floats, where any change of
    order would show: column f equals the F = 1 call on that column, and a row-strided view of X gives
    the bits of its contiguous copy."""
    g, ap, aj, aw = general_graph(ea, ctx, name)
    x = np.random.default_rng(6).standard_normal((g.n_cols, 37)).astype(np.float32)
    hook(monkeypatch, segment)
    y, _ = twice(ea, ctx, g, on_device(x))
    for f in range(37):
        column, _ = twice(ea, ctx, g, on_device(x[:, f:f + 1]))
        assert same_bits(column[:, 0], y[:, f]), f
    wide, _ = twice(ea, ctx, g, on_device(x, ld=41, offset=3), ld=40)
    assert same_bits(wide, y)


def test_chesapeake_within_the_summation_bound(ea, ctx):
    """|fl(sum) - sum| <= gamma(D + 1) * sum |terms| for D terms in ANY order (D - 1 additions and the
    products, fused or not; Higham, Accuracy and Stability, section 4.2): per element, with the row's
    own D."""
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, aw = g.to_host()
    x = np.random.default_rng(6).standard_normal((g.n_cols, 16)).astype(np.float32)
    y, _ = twice(ea, ctx, g, on_device(x))
    want = spmm(ap, aj, aw, x)
    magnitude = spmm(ap, aj, np.abs(aw), np.abs(x))
    bound = 1.01 * (np.diff(ap)[:, None] + 1) * 2.0 ** -24 * magnitude
    error = np.abs(y.astype(np.float64) - want)
    print(f"largest error / bound: {(error[bound > 0] / bound[bound > 0]).max():.3f}")
    assert (error <= bound).all()


# ---- transpose -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
def test_transpose_with_in_edges_on_a_directed_rmat(ea, ctx, monkeypatch, segment):
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    hook(monkeypatch, segment)
    x = integers(np.random.default_rng(5), (g.n_rows, 4))
    forward, _ = twice(ea, ctx, g, on_device(x))
    back, _ = twice(ea, ctx, g, on_device(x), transpose=True)
    assert (forward == exact(spmm(ap, aj, aw, x))).all()
    assert (back == exact(spmm(ap, aj, aw, x, transpose=True))).all()
    assert (forward != back).any()
    assert np.diff(transpose(ap, aj, aw)[0]).max() > 64  # an in-row that the hook at its minimum cuts


def test_transpose_uses_the_in_edge_values(ea, ctx):
    """Directed K4 with row weights {2, 1, 1}: the in-row of v holds the 2 of v - 1, which the out-row
    of v does not, and structurally the CSR is symmetric."""
    k4 = [(u, (u + d) % 4) for u in range(4) for d in (1, 2, 3)]
    ap, aj, aw = csr(4, k4, [2.0 if d == 1 else 1.0 for u in range(4) for d in (1, 2, 3)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw).build_in_edges(ctx)
    x = np.array([[1, 2], [10, 20], [100, 200], [1000, 2000]], np.float32)
    back, _ = twice(ea, ctx, g, on_device(x), transpose=True)
    assert back[:, 0].tolist() == [2110.0, 1102.0, 1021.0, 211.0] and (back[:, 1] == 2 * back[:, 0]).all()
    assert (back == exact(spmm(ap, aj, aw, x, transpose=True))).all()
    forward, _ = twice(ea, ctx, g, on_device(x))
    assert forward[:, 0].tolist() == [1120.0, 1201.0, 2011.0, 112.0] and (forward[:, 1] == 2 * forward[:, 0]).all()


def test_transpose_refusals(ea, ctx, ladder):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    x = torch.ones((4, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ea.EngineError) as e:
        ea.spmm(ctx, g, x, transpose=True)
    message = lib.grx_last_error()
    assert e.value.code == -3 and b"grx_spmm" in message and b"grx_graph_build_in_edges" in message
    y, _ = ea.spmm(ctx, g, x)  # the forward product needs nothing
    assert y.tolist() == [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0]]
    g.build_in_edges(ctx)
    y, _ = ea.spmm(ctx, g, x, transpose=True)
    assert y.tolist() == [[0.0, 0.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0]]
    wide = ea.Graph.from_host_csr(*ladder, n_cols=COLUMNS)
    with pytest.raises(ea.EngineError) as e:
        ea.spmm(ctx, wide, torch.ones((12, 2), dtype=torch.float32, device="cuda"), transpose=True)
    assert e.value.code == -3 and b"grx_spmm" in lib.grx_last_error()
    y, _ = ea.spmm(ctx, wide, torch.ones((COLUMNS, 2), dtype=torch.float32, device="cuda"))
    assert (y.cpu().numpy() == spmm(*ladder, np.ones((COLUMNS, 2)))).all()


# ---- values are read as they are -----------------------------------------------------------------------

def test_zero_weight_times_infinity_is_nan(ea, ctx):
    """Row 0 holds an entry of weight 0 whose feature 1 is inf: that element is NaN, and nothing else is."""
    ap, aj, aw = csr(3, [(0, 1), (0, 2), (1, 2), (2, 0)], weights=[0.0, 3.0, 2.0, 5.0], symmetric=False)
    x = np.array([[1, 2, 3], [4, np.inf, 6], [7, 8, 9]], np.float32)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    y, _ = twice(ea, ctx, g, on_device(x))
    assert np.isnan(y[0, 1])
    y[0, 1] = 0.0
    assert y.tolist() == [[21.0, 0.0, 27.0], [14.0, 16.0, 18.0], [5.0, 10.0, 15.0]]


# ---- edge cases and errors -----------------------------------------------------------------------------

def test_no_entries_writes_zeros(ea, ctx):
    ap, aj, aw = csr(5, [])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    for t in (False, True):  # without entries the CSR is its own transpose
        y, _ = twice(ea, ctx, g, on_device(np.ones((5, 3), np.float32)), transpose=t, ld=5)
        assert (y == 0).all() and y.shape == (5, 3) and not np.signbit(y).any()


def test_no_vertices_and_no_features(ea, ctx, rmat):
    import torch
    g = ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])
    y, st = ea.spmm(ctx, g, torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    assert y.shape == (0, 4) and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0
    y, st = ea.spmm(ctx, rmat[0], torch.empty((1024, 0), dtype=torch.float32, device="cuda"))
    assert y.shape == (1024, 0) and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0


def test_a_graph_below_one_segment_plans_nothing(ea, ctx, rmat):
    ap, aj, aw = csr(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], weights=[1, 2, 3, 4, 5, 6])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    y, st = twice(ea, ctx, g, on_device(x))
    assert (y == exact(spmm(ap, aj, aw, x))).all()
    _, planned = twice(ea, ctx, rmat[0], on_device(np.ones((1024, 2), np.float32)))
    assert st.advance_launches < planned.advance_launches


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    F = 2
    both = torch.ones(16, dtype=torch.float32, device="cuda")
    x, y = both[:8].view(4, F), both[8:].view(4, F)

    def call(c, h, px, py, features=F, ldx=F, ldy=F):
        return lib.grx_spmm(c, h, 0, features, px, ldx, py, ldy, None, None)

    def refused(*a, **k):
        return call(*a, **k) == -1 and b"grx_spmm" in lib.grx_last_error()

    assert refused(None, g._h, x.data_ptr(), y.data_ptr())
    assert refused(ctx._h, None, x.data_ptr(), y.data_ptr())
    assert refused(ctx._h, g._h, None, y.data_ptr())
    assert refused(ctx._h, g._h, x.data_ptr(), None)
    assert refused(ctx._h, g._h, x.data_ptr(), y.data_ptr(), features=-1)
    assert refused(ctx._h, g._h, x.data_ptr(), y.data_ptr(), ldx=1)
    assert refused(ctx._h, g._h, x.data_ptr(), y.data_ptr(), ldy=1)
    assert refused(ctx._h, g._h, x.data_ptr(), x.data_ptr()) and b"overlap" in lib.grx_last_error()
    assert refused(ctx._h, g._h, x.data_ptr(), both[7:15].data_ptr()) and b"overlap" in lib.grx_last_error()
    # the two halves of the rows of one [4, 4] buffer share no element, but their byte ranges interleave
    left, right = both.view(4, 4)[:, :F], both.view(4, 4)[:, F:]
    assert refused(ctx._h, g._h, left.data_ptr(), right.data_ptr(), ldx=4, ldy=4)
    assert b"overlap" in lib.grx_last_error()
    ctx.synchronize()
    assert (both == 1).all()  # nothing was launched
    assert call(ctx._h, g._h, x.data_ptr(), y.data_ptr()) == 0                # side by side is fine
    ctx.synchronize()
    assert y.tolist() == [[1.0, 1.0], [2.0, 2.0], [2.0, 2.0], [1.0, 1.0]] and (x == 1).all()
    with pytest.raises(TypeError):
        ea.spmm(ctx, g, x.double())
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, both[:4])                                             # one dimension
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, both[:8].view(F, 4).t())                              # stride(1) != 1
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, both[:6].view(3, F))                                  # three rows for four columns
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, x, y=both[8:14].view(3, F))                           # a short y


# ---- autograd ------------------------------------------------------------------------------------------

def test_autograd_backward_is_the_transposed_product(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    rng = np.random.default_rng(12)
    x = torch.from_numpy(integers(rng, (g.n_cols, 6))).cuda().requires_grad_()
    gy = integers(rng, (g.n_rows, 6))
    y = ea.spmm_autograd(ctx, g, x)
    assert y.requires_grad and (y.detach().cpu().numpy() == exact(spmm(ap, aj, aw, x.detach().cpu().numpy()))).all()
    y.backward(torch.from_numpy(gy).cuda())
    direct, _ = ea.spmm(ctx, g, torch.from_numpy(gy).cuda(), transpose=True)
    assert same_bits(x.grad.cpu().numpy(), direct.cpu().numpy())
    assert (x.grad.cpu().numpy() == exact(spmm(ap, aj, aw, gy, transpose=True))).all()


def test_autograd_raises_at_backward_time_without_in_edges(ea, ctx):
    import torch
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    x = torch.ones((4, 2), dtype=torch.float32, device="cuda", requires_grad=True)
    y = ea.spmm_autograd(ctx, g, x)  # forward needs nothing
    assert y.tolist() == [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0]]
    with pytest.raises(ea.EngineError):
        y.sum().backward()
