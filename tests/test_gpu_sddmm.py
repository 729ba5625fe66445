"""grx_sddmm (out[e] = <U[row(e)], V[col(e)]>: features on the lanes, the lanes' partials met in a written
butterfly) and grx_spmm_values (grx_spmm with the caller's per-entry values) against numpy: bit for bit
on integer inputs whose sums float32 holds exactly, bit for bit against the header's written order on
inputs that tell orders apart, within the standard summation bound on general floats, and the two as
each other's derivatives under autograd.  Every grx_sddmm call is made twice, into nnz floats inside a
storage filled with -7 and then NaN, and must repeat itself and leave the guards alone; operands are
device views whose padding is NaN.  Each case is named for what can go wrong at its shape."""
import os

import numpy as np
import pytest

import spmm_oracle
from sddmm_oracle import csr, order_inputs, sddmm, sddmm_in_order, sweep_ladder, transpose
from spmm_oracle import spmm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4096]  # test_gpu_spmm.py's: around a chunk of entries,
                                                             # the minimum segment and the default one
COLUMNS = 4096
SEGMENTS = [None, "64"]
GUARD = 3
INVALID, UNSUPPORTED = -1, -3  # GRX_ERR_INVALID_ARGUMENT, GRX_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def on_device(x, ld=None, offset=0):
    """The numpy matrix as a device view of row stride ld that begins `offset` floats into its storage;
    what lies between and around its rows is NaN, so reading it shows."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    rows, F = x.shape
    ld = ld or F
    storage = torch.full((offset + max(rows, 1) * ld,), float("nan"), dtype=torch.float32, device="cuda")
    view = storage[offset:offset + rows * ld].view(rows, ld)[:, :F]
    view.copy_(torch.from_numpy(x))
    return view


def vector_on_device(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def twice(ea, ctx, g, ud, vd):
    """Two calls of ea.sddmm into the middle of storages filled with something else: the second repeats
    the first bit for bit and neither touches the guards.  -> (out as a numpy array, Stats) of the first."""
    import torch
    first = None
    for fill in (-7.0, float("nan")):
        storage = torch.full((g.nnz + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
        out, st = ea.sddmm(ctx, g, ud, vd, out=storage[GUARD:GUARD + g.nnz])
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


def integers(rng, shape, below=16):
    return rng.integers(0, below, shape).astype(np.float32)


def exact(y64):
    """An integer result below 2**24 as the float32 it must be."""
    assert (y64 == np.round(y64)).all() and (np.abs(y64) < 2 ** 24).all()
    return y64.astype(np.float32)


@pytest.fixture(scope="module")
def rmat(ea, ctx):
    """2**10 vertices, symmetric: more than one sweep of a workgroup, empty rows, and hub rows that the
    hook at its minimum cuts into many items and the default into a few."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7)
    ap, aj, aw = g.to_host()
    degree = np.diff(ap)
    assert degree.max() > 512 and (degree == 0).any()
    assert aw.min() >= 1 and aw.max() <= 64 and (aw == np.round(aw)).all()
    return g, ap, aj, aw


@pytest.fixture(scope="module")
def directed(ea, ctx):
    """The directed R-MAT of the same size with its in-edges, and the same structure without them."""
    g = ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    g.build_in_edges(ctx)
    assert np.diff(transpose(ap, aj, aw)[0]).max() > 64  # an in-row that the hook at its minimum cuts
    return g, ap, aj, aw, ea.Graph.from_host_csr(ap, aj, aw)


@pytest.fixture(scope="module")
def ladder():
    rng = np.random.default_rng(11)
    ap = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.int32)
    aj = np.concatenate([rng.permutation(COLUMNS)[:d] for d in LADDER]).astype(np.int32)  # rows not sorted
    return ap, aj, np.ones(len(aj), np.float32)


def hook(monkeypatch, segment, name="GRX_SDDMM_SEGMENT"):
    if segment:
        monkeypatch.setenv(name, segment)


# ---- exact integer products: any order must give these bits -------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [1, 3, 4, 7, 64, 256, 260])
def test_exact_on_a_symmetric_rmat(ea, ctx, rmat, monkeypatch, F, segment):
    """One lane with one feature; a tail narrower than a vector; exactly one vector; two lanes, the
    second ragged; a quarter wavefront per row; a whole wavefront of full vectors; a second tile of one
    lane behind a full one."""
    g, ap, aj, _ = rmat
    rng = np.random.default_rng(3)
    u, v = integers(rng, (g.n_rows, F)), integers(rng, (g.n_cols, F))
    hook(monkeypatch, segment)
    out, st = twice(ea, ctx, g, on_device(u), on_device(v))
    assert (out == exact(sddmm(ap, aj, u, v))).all()
    assert st.advance_launches == 3  # the plan, the short rows, the items of the long ones


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [12, 20, 100])
def test_exact_at_the_other_group_widths(ea, ctx, rmat, monkeypatch, F, segment):
    """4, 8 and 32 lanes per row, which the list above does not reach."""
    g, ap, aj, _ = rmat
    rng = np.random.default_rng(13)
    u, v = integers(rng, (g.n_rows, F)), integers(rng, (g.n_cols, F))
    hook(monkeypatch, segment)
    out, _ = twice(ea, ctx, g, on_device(u), on_device(v))
    assert (out == exact(sddmm(ap, aj, u, v))).all()


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [5, 64])
def test_exact_on_a_rectangular_ladder(ea, ctx, ladder, monkeypatch, F, segment):
    """12 rows over 4096 columns, columns unsorted: every length at which a chunk of entries or a
    segment fills up, one below and one above; U has 12 rows and V 4096."""
    ap, aj, aw = ladder
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols=COLUMNS)
    assert (g.n_rows, g.n_cols) == (12, COLUMNS)
    rng = np.random.default_rng(4)
    u, v = integers(rng, (12, F)), integers(rng, (COLUMNS, F))
    hook(monkeypatch, segment)
    out, _ = twice(ea, ctx, g, on_device(u), on_device(v))
    want = exact(sddmm(ap, aj, u, v))
    assert (out == want).all(), np.argwhere(out != want)


@pytest.mark.parametrize("F", [5, 64])
def test_strided_and_misaligned_operands(ea, ctx, ladder, F):
    """U in rows F + 1 apart that begin 3 floats into their storage, V in rows F + 3 apart: no 16-byte
    access is possible, at F = 5 the second lane has a ragged tail, and what lies between the rows
    (NaN) is not read: the bits are the contiguous call's."""
    ap, aj, aw = ladder
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols=COLUMNS)
    rng = np.random.default_rng(5)
    u = rng.standard_normal((12, F)).astype(np.float32)
    v = rng.standard_normal((COLUMNS, F)).astype(np.float32)
    plain, _ = twice(ea, ctx, g, on_device(u), on_device(v))
    ud, vd = on_device(u, ld=F + 1, offset=3), on_device(v, ld=F + 3)
    assert ud.data_ptr() % 16 == 12 and ud.stride() == (F + 1, 1) and vd.stride() == (F + 3, 1)
    out, _ = twice(ea, ctx, g, ud, vd)
    assert not np.isnan(out).any() and same_bits(out, plain)
    mixed, _ = twice(ea, ctx, g, on_device(u), vd)  # one operand that could be read 16 bytes wide
    assert same_bits(mixed, plain)


# ---- the written order ---------------------------------------------------------------------------------

@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("F", [9, 37, 64, 260, 516])
def test_the_written_order(ea, ctx, monkeypatch, F, segment):
    """Features on which nearly every step rounds (tests/test_sddmm_abi.py shows that they tell the
    butterfly from a sequential sum and from a sequential sum of the lanes' partials): every bit is
    the header's order's.  Four lanes with a one-feature tail; sixteen with a ragged tenth; sixteen
    full; a second tile of one lane; a third tile of one lane behind two full ones."""
    lengths = [1, 64, 65, 200, 513, 1025]
    rng = np.random.default_rng(21)
    ap = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    aj = np.concatenate([rng.choice(2048, d, replace=False) for d in lengths]).astype(np.int32)
    u, v = order_inputs(rng, (len(lengths), F)), order_inputs(rng, (2048, F))
    g = ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols=2048)
    hook(monkeypatch, segment)
    out, _ = twice(ea, ctx, g, on_device(u), on_device(v))
    want = sddmm_in_order(ap, aj, u, v, "tree")
    assert same_bits(out, want), np.argwhere(out.view(np.uint32) != want.view(np.uint32))[:8]


def general_graph(ea, name):
    if name == "chesapeake":
        g = ea.Graph.from_mtx(CHESAPEAKE)
        return (g,) + tuple(g.to_host())
    ap, aj, aw = sweep_ladder()
    return ea.Graph.from_host_csr(ap, aj, aw), ap, aj, aw


@pytest.mark.parametrize("name", ["chesapeake", "sweep_ladder"])
def test_the_order_does_not_notice_the_layout(ea, ctx, monkeypatch, name):
    """F = 37 on general floats, where any change of order would show: the hook at 64 gives the default's
    bits, the repeats of a column within a row get equal results, and every row's results are those of
    a graph that holds nothing but that row."""
    g, ap, aj, aw = general_graph(ea, name)
    rng = np.random.default_rng(6)
    u = rng.standard_normal((g.n_rows, 37)).astype(np.float32)
    v = rng.standard_normal((g.n_cols, 37)).astype(np.float32)
    ud, vd = on_device(u), on_device(v)
    out, _ = twice(ea, ctx, g, ud, vd)
    repeats = 0
    for r in range(g.n_rows):
        cols, mine = aj[ap[r]:ap[r + 1]], out[ap[r]:ap[r + 1]]
        for c in np.unique(cols):
            at = np.flatnonzero(cols == c)
            repeats += len(at) - 1
            assert same_bits(mine[at], np.repeat(mine[at[:1]], len(at))), (r, c)
        if len(cols) == 0:
            continue
        alone = ea.Graph.from_host_csr(np.array([0, len(cols)], np.int32), cols, np.ones(len(cols), np.float32),
                                       n_cols=g.n_cols)
        single, _ = twice(ea, ctx, alone, ud[r:r + 1], vd)
        assert same_bits(single, mine), r
    assert repeats > 0 or name == "chesapeake"  # the sweep ladder is a multigraph
    hook(monkeypatch, "64")
    cut, _ = twice(ea, ctx, g, ud, vd)
    assert same_bits(cut, out)


# ---- general floats ------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [16, 300])
def test_chesapeake_within_the_summation_bound(ea, ctx, F):
    """|fl(sum) - sum| <= gamma(D + 1) * sum |terms| for D terms in ANY order (D - 1 additions and the
    products, fused or not; Higham, Accuracy and Stability, section 4.2): per entry, with D = F."""
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    rng = np.random.default_rng(6)
    u = rng.standard_normal((g.n_rows, F)).astype(np.float32)
    v = rng.standard_normal((g.n_cols, F)).astype(np.float32)
    out, _ = twice(ea, ctx, g, on_device(u), on_device(v))
    want = sddmm(ap, aj, u, v)
    bound = 1.01 * (F + 1) * 2.0 ** -24 * sddmm(ap, aj, np.abs(u), np.abs(v))
    error = np.abs(out.astype(np.float64) - want)
    print(f"F = {F}: largest error / bound: {(error[bound > 0] / bound[bound > 0]).max():.3f}")
    assert (error <= bound).all()


# ---- grx_spmm_values -----------------------------------------------------------------------------------

def product(ea, ctx, g, x, transpose=False, values=None):
    """ea.spmm twice -> Y of the first call as a numpy array; the second has its bits."""
    y, _ = ea.spmm(ctx, g, on_device(x), transpose=transpose, values=values)
    again, _ = ea.spmm(ctx, g, on_device(x), transpose=transpose, values=values)
    assert same_bits(y.cpu().numpy(), again.cpu().numpy())
    return y.cpu().numpy()


def refused_without_in_edges(ea, ctx, g, values):
    import torch
    from essentials_amd.api import load_library
    x = torch.ones((g.n_rows, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ea.EngineError) as e:
        ea.spmm(ctx, g, x, transpose=True, values=values)
    message = load_library().grx_last_error()
    return e.value.code == UNSUPPORTED and b"grx_spmm_values" in message and b"grx_graph_build_in_edges" in message


def values_against_a_second_handle(ea, ctx, monkeypatch, g, second, ap, aj, aw, w2, t):
    """The three comparisons of grx_spmm_values, forward or transposed."""
    rng = np.random.default_rng(31)
    wd, w2d = vector_on_device(aw), vector_on_device(w2)
    x = integers(rng, (g.n_rows, 6))
    own = product(ea, ctx, g, x, t)
    assert (own == exact(spmm(ap, aj, aw, x, transpose=t))).all()
    assert same_bits(product(ea, ctx, g, x, t, values=wd), own)  # the handle's own values, passed in
    other = product(ea, ctx, g, x, t, values=w2d)
    assert same_bits(other, product(ea, ctx, second, x, t))
    assert (other == exact(spmm(ap, aj, w2, x, transpose=t))).all() and (other != own).any()
    rough = spmm_oracle.order_inputs(rng, (g.n_rows, 5))
    for segment in SEGMENTS:
        with monkeypatch.context() as m:
            hook(m, segment, "GRX_SPMM_SEGMENT")
            assert same_bits(product(ea, ctx, g, rough, t, values=wd), product(ea, ctx, g, rough, t)), segment
            assert same_bits(product(ea, ctx, g, rough, t, values=w2d), product(ea, ctx, second, rough, t)), segment


def test_spmm_values_forward(ea, ctx, rmat, monkeypatch):
    """With its own values the call has grx_spmm's bits, on integers and on features that tell orders
    apart under both segment sizes; with other values those of a handle built with them."""
    g, ap, aj, aw = rmat
    w2 = np.random.default_rng(32).integers(1, 65, len(aw)).astype(np.float32)
    assert (w2 != aw).any()
    values_against_a_second_handle(ea, ctx, monkeypatch, g, ea.Graph.from_host_csr(ap, aj, w2), ap, aj, aw, w2, False)
    # symmetric, so grx_spmm's transposed product walks the rows; a caller's values have no mirror image
    assert refused_without_in_edges(ea, ctx, g, vector_on_device(aw))


def test_spmm_values_transposed(ea, ctx, directed, monkeypatch):
    """The values follow their entries into the in-rows through the entry ids of the in-edges."""
    g, ap, aj, aw, bare = directed
    w2 = np.random.default_rng(33).integers(1, 65, len(aw)).astype(np.float32)
    second = ea.Graph.from_host_csr(ap, aj, w2).build_in_edges(ctx)
    values_against_a_second_handle(ea, ctx, monkeypatch, g, second, ap, aj, aw, w2, True)
    assert refused_without_in_edges(ea, ctx, bare, vector_on_device(aw))


def test_spmm_values_on_the_directed_k4(ea, ctx):
    """test_transpose_uses_the_in_edge_values' numbers, with the row weights {2, 1, 1} passed by the
    caller on a handle built with ones."""
    k4 = [(u, (u + d) % 4) for u in range(4) for d in (1, 2, 3)]
    ap, aj, ones = csr(4, k4, symmetric=False)
    w = vector_on_device([2.0 if d == 1 else 1.0 for u in range(4) for d in (1, 2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, ones).build_in_edges(ctx)
    x = np.array([[1, 2], [10, 20], [100, 200], [1000, 2000]], np.float32)
    back = product(ea, ctx, g, x, True, values=w)
    assert back[:, 0].tolist() == [2110.0, 1102.0, 1021.0, 211.0] and (back[:, 1] == 2 * back[:, 0]).all()
    forward = product(ea, ctx, g, x, False, values=w)
    assert forward[:, 0].tolist() == [1120.0, 1201.0, 2011.0, 112.0] and (forward[:, 1] == 2 * forward[:, 0]).all()
    assert product(ea, ctx, g, x, True)[:, 0].tolist() == [1110.0, 1101.0, 1011.0, 111.0]  # the handle's ones


# ---- refusals ------------------------------------------------------------------------------------------

def test_sddmm_refusals(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    F = 2
    all_of_it = torch.ones(16 + 6, dtype=torch.float32, device="cuda")
    u, v, out = all_of_it[:8].view(4, F), all_of_it[8:16].view(4, F), all_of_it[16:]
    assert g.nnz == 6

    def call(c, h, pu, pv, po, features=F, ldu=F, ldv=F):
        return lib.grx_sddmm(c, h, features, pu, ldu, pv, ldv, po, None, None)

    def refused(*a, **k):
        return call(*a, **k) == INVALID and b"grx_sddmm" in lib.grx_last_error()

    p = (u.data_ptr(), v.data_ptr(), out.data_ptr())
    assert refused(None, g._h, *p)
    assert refused(ctx._h, None, *p)
    assert refused(ctx._h, g._h, None, p[1], p[2])
    assert refused(ctx._h, g._h, p[0], None, p[2])
    assert refused(ctx._h, g._h, p[0], p[1], None)
    assert refused(ctx._h, g._h, *p, features=-1)
    assert refused(ctx._h, g._h, *p, ldu=1)
    assert refused(ctx._h, g._h, *p, ldv=1)
    assert refused(ctx._h, g._h, p[0], p[1], p[0]) and b"overlap" in lib.grx_last_error()
    assert refused(ctx._h, g._h, p[0], p[1], all_of_it[7:].data_ptr()) and b"overlap" in lib.grx_last_error()
    assert refused(ctx._h, g._h, p[0], p[1], all_of_it[15:].data_ptr()) and b"overlap" in lib.grx_last_error()
    ctx.synchronize()
    assert (all_of_it == 1).all()  # nothing was launched
    assert call(ctx._h, g._h, p[0], p[0], p[2]) == 0  # U and V may be one matrix; side by side is fine
    ctx.synchronize()
    assert out.tolist() == [2.0] * 6 and (all_of_it[:16] == 1).all()
    with pytest.raises(TypeError):
        ea.sddmm(ctx, g, u.double(), v)
    with pytest.raises(ValueError):
        ea.sddmm(ctx, g, u, all_of_it[:12].view(4, 3))                        # another F
    with pytest.raises(ValueError):
        ea.sddmm(ctx, g, all_of_it[:6].view(3, F), v)                         # three rows for four
    with pytest.raises(ValueError):
        ea.sddmm(ctx, g, u, v, out=all_of_it[:5])                             # a short out
    with pytest.raises(ValueError):
        ea.sddmm(ctx, g, u, v, out=all_of_it[::2][:6])                        # not contiguous
    with pytest.raises(ea.EngineError) as e:
        ea.sddmm(ctx, g, u, v, out=all_of_it[6:12])
    assert e.value.code == INVALID


def test_spmm_values_refusals(ea, ctx, rmat, ladder):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    F = 2
    x = torch.ones((4, F), dtype=torch.float32, device="cuda")
    storage = torch.ones(6 + 8, dtype=torch.float32, device="cuda")
    w = storage[:6]
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, x, values=storage[:5])                                # the wrong length
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, x, values=storage[:12][::2])                          # not contiguous
    with pytest.raises(TypeError):
        ea.spmm(ctx, g, x, values=w.double())
    with pytest.raises(ValueError):
        ea.spmm(ctx, g, x, values=w.cpu())
    with pytest.raises(ea.EngineError) as e:
        ea.spmm(ctx, g, x, values=w, y=storage[5:13].view(4, F))              # the last value is y[0, 0]
    message = lib.grx_last_error()
    assert e.value.code == INVALID and b"grx_spmm_values" in message and b"overlap" in message
    y = torch.zeros((4, F), dtype=torch.float32, device="cuda")
    rc = lib.grx_spmm_values(ctx._h, g._h, None, 0, F, x.data_ptr(), F, y.data_ptr(), F, None, None)
    assert rc == INVALID and b"grx_spmm_values" in lib.grx_last_error()
    rc = lib.grx_spmm_values(ctx._h, g._h, w.data_ptr(), 0, F, x.data_ptr(), 1, y.data_ptr(), F, None, None)
    assert rc == INVALID and b"grx_spmm_values" in lib.grx_last_error()       # grx_spmm's list, under this name
    ctx.synchronize()
    assert (y == 0).all() and (storage == 1).all()  # nothing was launched
    out, _ = ea.spmm(ctx, g, x, values=w, y=storage[6:].view(4, F))           # side by side is fine
    assert out.tolist() == [[1.0, 1.0], [2.0, 2.0], [2.0, 2.0], [1.0, 1.0]]
    # transposed: a symmetric handle without in-edges, and a rectangular one
    assert refused_without_in_edges(ea, ctx, g, storage[:6])
    assert refused_without_in_edges(ea, ctx, rmat[0], vector_on_device(rmat[3]))
    wide = ea.Graph.from_host_csr(*ladder, n_cols=COLUMNS)
    with pytest.raises(ea.EngineError) as e:
        ea.spmm(ctx, wide, torch.ones((12, F), dtype=torch.float32, device="cuda"), transpose=True,
                values=vector_on_device(ladder[2]))
    assert e.value.code == UNSUPPORTED and b"grx_spmm_values" in lib.grx_last_error()


# ---- empty shapes --------------------------------------------------------------------------------------

def test_no_features_gives_zeros(ea, ctx, rmat):
    g = rmat[0]
    out, st = twice(ea, ctx, g, on_device(np.zeros((g.n_rows, 0), np.float32)),
                    on_device(np.zeros((g.n_cols, 0), np.float32)))
    assert (out == 0).all() and not np.signbit(out).any() and st.advance_launches == 0


def test_no_entries_launches_nothing(ea, ctx):
    import torch
    ap, aj, aw = csr(5, [])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    u = torch.ones((5, 3), dtype=torch.float32, device="cuda")
    out, st = ea.sddmm(ctx, g, u, u)
    assert out.shape == (0,) and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0
    none = ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])
    out, st = ea.sddmm(ctx, none, u[:0], u[:0])
    assert out.shape == (0,) and st.advance_launches == 0 and st.elapsed_ms == 0 and st.iterations == 0


def test_a_graph_below_one_segment_plans_nothing(ea, ctx):
    ap, aj, aw = csr(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    u = np.arange(12, dtype=np.float32).reshape(6, 2)
    out, st = twice(ea, ctx, g, on_device(u), on_device(u))
    assert (out == exact(sddmm(ap, aj, u, u))).all() and st.advance_launches == 1


# ---- autograd ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_directed(ea, ctx):
    g = ea.Graph.rmat(ctx, 8, 16, 1, 7, symmetrize=False)
    ap, aj, aw = g.to_host()
    return g.build_in_edges(ctx), ap, aj, ea.Graph.from_host_csr(ap, aj, aw)


def leaf(x, grad=True):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().requires_grad_(grad)


def test_autograd_of_the_product_in_both_inputs(ea, ctx, small_directed):
    """d/dx of sum(T * (A(w) x)) is A(w)^T T and d/dw[e] is <T[row(e)], x[col(e)]>: integers, exactly."""
    import torch
    g, ap, aj, bare = small_directed
    rng = np.random.default_rng(41)
    x, w, T = integers(rng, (g.n_cols, 5), 8), integers(rng, g.nnz, 8), integers(rng, (g.n_rows, 5), 8)
    xd, wd = leaf(x), leaf(w)
    y = ea.spmm_autograd(ctx, g, xd, values=wd)
    assert y.requires_grad and (y.detach().cpu().numpy() == exact(spmm(ap, aj, w, x))).all()
    (y * torch.from_numpy(T).cuda()).sum().backward()
    assert (xd.grad.cpu().numpy() == exact(spmm(ap, aj, w, T, transpose=True))).all()
    assert (wd.grad.cpu().numpy() == exact(sddmm(ap, aj, T, x))).all()
    # one input at a time: the other gets no gradient, and the values' own needs no in-edges
    xd, wd = leaf(x), leaf(w, False)
    (ea.spmm_autograd(ctx, g, xd, values=wd) * torch.from_numpy(T).cuda()).sum().backward()
    assert wd.grad is None and (xd.grad.cpu().numpy() == exact(spmm(ap, aj, w, T, transpose=True))).all()
    xd, wd = leaf(x, False), leaf(w)
    (ea.spmm_autograd(ctx, bare, xd, values=wd) * torch.from_numpy(T).cuda()).sum().backward()
    assert xd.grad is None and (wd.grad.cpu().numpy() == exact(sddmm(ap, aj, T, x))).all()
    xd, wd = leaf(x), leaf(w)
    with pytest.raises(ea.EngineError):
        ea.spmm_autograd(ctx, bare, xd, values=wd).sum().backward()  # x's gradient is the transposed product


def test_autograd_of_the_scores_in_both_inputs(ea, ctx, small_directed):
    """d/du of sum(T * sddmm(u, v)) is A(T) v and d/dv is A(T)^T u."""
    import torch
    g, ap, aj, bare = small_directed
    rng = np.random.default_rng(42)
    u, v, T = integers(rng, (g.n_rows, 5), 8), integers(rng, (g.n_cols, 5), 8), integers(rng, g.nnz, 8)
    ud, vd = leaf(u), leaf(v)
    s = ea.sddmm_autograd(ctx, g, ud, vd)
    assert s.requires_grad and (s.detach().cpu().numpy() == exact(sddmm(ap, aj, u, v))).all()
    (s * torch.from_numpy(T).cuda()).sum().backward()
    assert (ud.grad.cpu().numpy() == exact(spmm(ap, aj, T, v))).all()
    assert (vd.grad.cpu().numpy() == exact(spmm(ap, aj, T, u, transpose=True))).all()
    ud, vd = leaf(u), leaf(v, False)
    (ea.sddmm_autograd(ctx, bare, ud, vd) * torch.from_numpy(T).cuda()).sum().backward()  # no in-edges needed
    assert vd.grad is None and (ud.grad.cpu().numpy() == exact(spmm(ap, aj, T, v))).all()
    ud, vd = leaf(u, False), leaf(v)
    with pytest.raises(ea.EngineError):
        ea.sddmm_autograd(ctx, bare, ud, vd).sum().backward()  # v's gradient is the transposed product


def test_autograd_without_values_is_unchanged(ea, ctx, small_directed):
    import torch
    g, ap, aj, _ = small_directed
    aw = g.to_host()[2]
    rng = np.random.default_rng(43)
    x, T = integers(rng, (g.n_cols, 5), 8), integers(rng, (g.n_rows, 5), 8)
    xd = leaf(x)
    y = ea.spmm_autograd(ctx, g, xd)
    assert same_bits(y.detach().cpu().numpy(), ea.spmm(ctx, g, xd.detach())[0].cpu().numpy())
    y.backward(torch.from_numpy(T).cuda())
    assert (xd.grad.cpu().numpy() == exact(spmm(ap, aj, aw, T, transpose=True))).all()
