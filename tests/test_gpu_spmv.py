"""grx_spmv (row sums in a fixed order by 16-lane groups, long rows cut into segments) against numpy:
bit for bit on integer inputs whose sums float32 holds exactly, within the standard summation bound on
general floats.  Every call is made twice and must repeat itself.  Each case is named for what can go
wrong at its shape."""
import os

import numpy as np
import pytest

from hits_oracle import SWEEP_LENGTHS, csr, spmv, sweep_ladder, transpose

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4096]  # row lengths around the group, the minimum
                                                             # segment and the default one
COLUMNS = 4096


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def twice(ea, ctx, g, x, transpose=False):
    """Two calls of ea.spmv into tensors filled with something else: the second repeats the first bit
    for bit.  -> (y as a numpy array, Stats) of the first."""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    first = None
    for fill in (-7.0, float("nan")):
        y = torch.full((g.n_cols if transpose else g.n_rows,), fill, dtype=torch.float32, device="cuda")
        out, st = ea.spmv(ctx, g, xd, transpose=transpose, y=y)
        assert out.data_ptr() == y.data_ptr()
        assert st.iterations == 1 and st.edges_traversed == st.edges_expanded == g.nnz
        assert st.advance_launches >= 1 and st.elapsed_ms > 0
        if first is None:
            first = (out.cpu().numpy(), st)
        else:
            assert (out.cpu().numpy().view(np.uint32) == first[0].view(np.uint32)).all()
            assert st.advance_launches == first[1].advance_launches
    return first


def integers(rng, n):
    return rng.integers(0, 16, n).astype(np.float32)


def exact(y64):
    """An integer product below 2**24 as the float32 it must be."""
    assert (y64 == np.round(y64)).all() and (np.abs(y64) < 2 ** 24).all()
    return y64.astype(np.float32)


@pytest.fixture(scope="module")
def ladder():
    rng = np.random.default_rng(11)
    ap = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.int32)
    aj = np.concatenate([rng.permutation(COLUMNS)[:d] for d in LADDER]).astype(np.int32)  # rows not sorted
    aw = rng.integers(1, 65, len(aj)).astype(np.float32)
    return ap, aj, aw


# ---- exact integer products: any order must give these bits -------------------------------------------

@pytest.mark.parametrize("segment", [None, "64"])
def test_exact_on_a_symmetric_rmat(ea, ctx, monkeypatch, segment):
    """2**10 vertices: more than one sweep of a workgroup's 16 rows, empty rows, and hub rows that the
    hook at its minimum cuts into many segments and the default into a few."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7)
    ap, aj, aw = g.to_host()
    degree = np.diff(ap)
    assert degree.max() > 512 and degree.max() <= 17000 and (degree == 0).any()
    assert aw.min() >= 1 and aw.max() <= 64 and (aw == np.round(aw)).all()
    x = integers(np.random.default_rng(3), g.n_cols)
    if segment:
        monkeypatch.setenv("GRX_SPMV_SEGMENT", segment)
    y, st = twice(ea, ctx, g, x)
    assert (y == exact(spmv(ap, aj, aw, x))).all()
    assert st.advance_launches == 4  # the plan, the short rows, the segments, their sums
    # symmetric, no in-edges: the transposed product walks the same rows
    back, _ = twice(ea, ctx, g, x, transpose=True)
    assert (back.view(np.uint32) == y.view(np.uint32)).all()


@pytest.mark.parametrize("segment", [None, "64"])
def test_exact_on_a_rectangular_ladder(ea, ctx, ladder, monkeypatch, segment):
    """12 rows over 4096 columns: every length at which a lane, a group or a segment fills up, one
    below and one above; 12 is no multiple of the 16 rows of a workgroup."""
    ap, aj, aw = ladder
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols=COLUMNS)
    assert (g.n_rows, g.n_cols) == (12, COLUMNS)
    x = integers(np.random.default_rng(4), COLUMNS)
    if segment:
        monkeypatch.setenv("GRX_SPMV_SEGMENT", segment)
    y, _ = twice(ea, ctx, g, x)
    want = exact(spmv(ap, aj, aw, x))
    assert (y == want).all(), (y, want)
    assert y[0] == 0 and (y[1:] > 0).all()


@pytest.mark.parametrize("segment", [None, "64"])
def test_exact_on_the_sweep_ladder(ea, ctx, monkeypatch, segment):
    """37 rows, out-rows forward and in-rows transposed: the last sweep of a workgroup has lane groups
    past the end, and under the hook a row of 64 is short, 65 leaves an item of one entry and 200 a
    partial last item; by default nothing is long but the plan still runs (776 entries)."""
    ap, aj, aw = sweep_ladder()
    for offsets in (ap, transpose(ap, aj, aw)[0]):
        assert len(offsets) == 38 and set(SWEEP_LENGTHS) <= set(np.diff(offsets).tolist())
    g = ea.Graph.from_host_csr(ap, aj, aw).build_in_edges(ctx)
    x = integers(np.random.default_rng(8), 37)
    if segment:
        monkeypatch.setenv("GRX_SPMV_SEGMENT", segment)
    forward, st = twice(ea, ctx, g, x)
    back, st_back = twice(ea, ctx, g, x, transpose=True)
    assert (forward == exact(spmv(ap, aj, aw, x))).all()
    assert (back == exact(spmv(ap, aj, aw, x, transpose=True))).all()
    assert st.advance_launches == st_back.advance_launches == 4


def test_a_graph_below_one_segment_plans_nothing(ea, ctx):
    ap, aj, aw = csr(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], weights=[1, 2, 3, 4, 5, 6])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    x = np.arange(6, dtype=np.float32)
    y, st = twice(ea, ctx, g, x)
    assert (y == exact(spmv(ap, aj, aw, x))).all() and st.advance_launches == 1


# ---- transpose -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", [None, "64"])
def test_transpose_with_in_edges_on_a_directed_rmat(ea, ctx, monkeypatch, segment):
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    if segment:
        monkeypatch.setenv("GRX_SPMV_SEGMENT", segment)
    x = integers(np.random.default_rng(5), g.n_rows)
    forward, _ = twice(ea, ctx, g, x)
    back, _ = twice(ea, ctx, g, x, transpose=True)
    assert (forward == exact(spmv(ap, aj, aw, x))).all()
    assert (back == exact(spmv(ap, aj, aw, x, transpose=True))).all()
    assert (forward != back).any()
    assert np.diff(transpose(ap, aj, aw)[0]).max() > 64  # an in-row that the hook at its minimum cuts


def test_transpose_uses_the_in_edge_values(ea, ctx):
    """Directed K4 with row weights {2, 1, 1}: the in-row of v holds the 2 of v - 1, which the out-row
    of v does not, and structurally the CSR is symmetric."""
    k4 = [(u, (u + d) % 4) for u in range(4) for d in (1, 2, 3)]
    ap, aj, aw = csr(4, k4, [2.0 if d == 1 else 1.0 for u in range(4) for d in (1, 2, 3)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw).build_in_edges(ctx)
    x = np.array([1, 10, 100, 1000], np.float32)
    back, _ = twice(ea, ctx, g, x, transpose=True)
    assert back.tolist() == [2110.0, 1102.0, 1021.0, 211.0]
    assert (back == exact(spmv(ap, aj, aw, x, transpose=True))).all()
    forward, _ = twice(ea, ctx, g, x)
    assert forward.tolist() == [1120.0, 1201.0, 2011.0, 112.0]


def test_transpose_refusals(ea, ctx, ladder):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    x = torch.ones(4, dtype=torch.float32, device="cuda")
    with pytest.raises(ea.EngineError) as e:
        ea.spmv(ctx, g, x, transpose=True)
    message = lib.grx_last_error()
    assert e.value.code == -3 and b"grx_spmv" in message and b"grx_graph_build_in_edges" in message
    y, _ = ea.spmv(ctx, g, x)  # the forward product needs nothing
    assert y.tolist() == [1.0, 1.0, 1.0, 0.0]
    g.build_in_edges(ctx)
    y, _ = ea.spmv(ctx, g, x, transpose=True)
    assert y.tolist() == [0.0, 1.0, 1.0, 1.0]
    wide = ea.Graph.from_host_csr(*ladder, n_cols=COLUMNS)
    with pytest.raises(ea.EngineError) as e:
        ea.spmv(ctx, wide, torch.ones(12, dtype=torch.float32, device="cuda"), transpose=True)
    assert e.value.code == -3 and b"grx_spmv" in lib.grx_last_error()


# ---- general floats ------------------------------------------------------------------------------------

def test_chesapeake_within_the_summation_bound(ea, ctx):
    """|fl(sum) - sum| <= gamma(D + 1) * sum |terms| for D terms in ANY order (D - 1 additions and the
    products, fused or not; Higham, Accuracy and Stability, section 4.2): per row, with the row's own D."""
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, aw = g.to_host()
    x = np.random.default_rng(6).standard_normal(g.n_cols).astype(np.float32)
    y, _ = twice(ea, ctx, g, x)
    want = spmv(ap, aj, aw, x)
    magnitude = spmv(ap, aj, np.abs(aw), np.abs(x))
    bound = 1.01 * (np.diff(ap) + 1) * 2.0 ** -24 * magnitude
    error = np.abs(y.astype(np.float64) - want)
    print(f"largest error / bound: {(error / bound).max():.3f}")
    assert (error <= bound).all()


# ---- edge cases and errors -----------------------------------------------------------------------------

def test_no_entries_writes_zeros(ea, ctx):
    ap, aj, aw = csr(5, [])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    for t in (False, True):  # without entries the CSR is its own transpose
        y, _ = twice(ea, ctx, g, np.ones(5, np.float32), transpose=t)
        assert y.tolist() == [0.0] * 5


def test_no_vertices(ea, ctx):
    import torch
    g = ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])
    y, st = ea.spmv(ctx, g, torch.empty(0, dtype=torch.float32, device="cuda"))
    assert y.numel() == 0 and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0


def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    both = torch.ones(8, dtype=torch.float32, device="cuda")
    x, y = both[:4], both[4:]

    def call(c, h, px, py):
        return lib.grx_spmv(c, h, 0, px, py, None, None)

    assert call(None, g._h, x.data_ptr(), y.data_ptr()) == -1
    assert call(ctx._h, None, x.data_ptr(), y.data_ptr()) == -1
    assert call(ctx._h, g._h, None, y.data_ptr()) == -1 and b"grx_spmv" in lib.grx_last_error()
    assert call(ctx._h, g._h, x.data_ptr(), None) == -1 and b"grx_spmv" in lib.grx_last_error()
    assert call(ctx._h, g._h, x.data_ptr(), x.data_ptr()) == -1 and b"overlap" in lib.grx_last_error()
    assert call(ctx._h, g._h, x.data_ptr(), both[3:7].data_ptr()) == -1       # one element shared
    assert call(ctx._h, g._h, both[1:5].data_ptr(), both[4:].data_ptr()) == -1
    ctx.synchronize()
    assert (both == 1).all()  # nothing was launched
    assert call(ctx._h, g._h, x.data_ptr(), y.data_ptr()) == 0                # side by side is fine
    ctx.synchronize()
    assert y.tolist() == [1.0, 2.0, 2.0, 1.0] and (x == 1).all()
    with pytest.raises(TypeError):
        ea.spmv(ctx, g, x.double())
    with pytest.raises(ValueError):
        ea.spmv(ctx, g, both)
    with pytest.raises(ValueError):
        ea.spmv(ctx, g, x, y=both[:3])
