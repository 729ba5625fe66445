"""grx_spgemm (C = A * B as a new handle) against the numpy oracle of tests/spgemm_oracle.py: the
reference's known pair, shapes that can go wrong, R-MAT products with integer weights (exact),
associativity and the result as an ordinary handle, the test hooks that force the other paths,
float weights against the float64 sum, 64-bit counting, stats, argument errors, and invariants on
RMAT-14 checked with torch and the engine's other calls."""
import ctypes as C

import numpy as np
import pytest

from spgemm_oracle import KNOWN, csr, product

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

HOOKS = ("GRX_SPGEMM_LDS_SLOTS", "GRX_SPGEMM_SMALL_PRODUCTS")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)


def graph(ea, m, n_cols):
    ap, aj, ax = m
    return ea.Graph.from_host_csr(ap, aj, ax, n_cols)


def arrays(ea, ctx, a, b, options=None):
    """(cp, cj, cx, Stats) of a * b on the host."""
    c, st = ea.spgemm(ctx, a, b, options)
    assert c.n_rows == a.n_rows and c.n_cols == b.n_cols and c.nnz == st.edges_traversed
    return (*c.to_host(), st)


def same(got, want):
    return all(g.shape == w.shape and (g == w).all() for g, w in zip(got[:3], want[:3]))


def check_exact(ea, ctx, A, B, n_mid, n_cols, a=None, b=None):
    """a * b equals the oracle's product of the host matrices A (? x n_mid) and B (n_mid x n_cols),
    whose partial sums are all representable."""
    cp, cj, cx64, terms, abs_sum, products = product(*A, *B, n_cols)
    assert not len(abs_sum) or abs_sum.max() < 2 ** 24
    a = a or graph(ea, A, n_mid)
    b = b or graph(ea, B, n_cols)
    gp, gj, gx, st = arrays(ea, ctx, a, b)
    assert gp.tolist() == cp.tolist()
    assert (gj == cj).all()
    assert gx.dtype == np.float32 and (gx == cx64.astype(np.float32)).all()
    assert st.edges_expanded == products and st.edges_traversed == len(cj)
    return (gp, gj, gx), (cp, cj, cx64, terms, abs_sum, products), st


def host(g):
    ap, aj, ax = g.to_host()
    return ap, aj.copy(), ax.copy()


_RMAT = {}


def rmat(ea, ctx, scale, ef=8, seed=1, weight_seed=7, symmetrize=True):
    """(Graph, its host arrays), built once per module."""
    key = (scale, ef, seed, weight_seed, symmetrize)
    if key not in _RMAT:
        g = ea.Graph.rmat(ctx, scale, ef, seed, weight_seed, symmetrize)
        _RMAT[key] = (g, host(g))
    return _RMAT[key]


_SQUARE = {}


def rmat10_square(ea, ctx):
    """R-MAT-10 with weights times itself: the default run's arrays and the oracle's, once."""
    if not _SQUARE:
        g, m = rmat(ea, ctx, 10)
        _SQUARE["got"], _SQUARE["want"], _SQUARE["stats"] = check_exact(ea, ctx, m, m, g.n_rows, g.n_cols, g, g)
    return _SQUARE["got"], _SQUARE["want"], _SQUARE["stats"]


def dense_pair():
    """64 x 1 times 1 x 40000: every row of C is dense and wider than any LDS table."""
    A = csr(64, 1, [(i, 0, float(1 + i % 3)) for i in range(64)])
    B = (np.array([0, 40000], np.int32), np.arange(40000, dtype=np.int32)[::-1].copy(),
         (1 + np.arange(40000) % 5).astype(np.float32))
    return A, B


# ---- 1. the known answer ---------------------------------------------------------------------------

def test_known_answer(ea, ctx):
    A, B = csr(*KNOWN["A"]), csr(*KNOWN["B"])
    (gp, gj, gx), _, st = check_exact(ea, ctx, A, B, 3, 3)
    want_p, want_j, want_x = KNOWN["C"]
    assert gp.tolist() == want_p and gj.tolist() == want_j and gx.tolist() == want_x
    assert st.edges_expanded == 5 and st.vertices_reached == 2


# ---- 2. shapes that can go wrong -------------------------------------------------------------------

def _empty(n_rows):
    return np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def test_zero_by_zero(ea, ctx):
    (gp, gj, _), _, st = check_exact(ea, ctx, _empty(0), _empty(0), 0, 0)
    assert gp.tolist() == [0] and len(gj) == 0 and st.vertices_reached == 0


def test_operands_without_entries(ea, ctx):
    (gp, gj, _), _, st = check_exact(ea, ctx, _empty(7), _empty(4), 4, 9)
    assert gp.tolist() == [0] * 8 and len(gj) == 0 and st.edges_expanded == 0
    # one side with entries, and no columns at all on the other
    A = csr(3, 4, [(0, 1, 2.0), (2, 3, 1.0)])
    check_exact(ea, ctx, A, _empty(4), 4, 0)
    check_exact(ea, ctx, A, _empty(4), 4, 6)


def test_three_by_five_by_two(ea, ctx):
    A = csr(3, 5, [(0, 4, 1.0), (0, 0, 2.0), (0, 4, 3.0), (2, 1, -1.0), (2, 2, 5.0)])
    B = csr(5, 2, [(0, 1, 1.0), (1, 0, 2.0), (2, 0, 3.0), (4, 1, 4.0), (4, 0, 1.0), (3, 1, 9.0)])
    (gp, gj, gx), _, _ = check_exact(ea, ctx, A, B, 5, 2)
    assert gp.tolist() == [0, 2, 2, 3] and gj.tolist() == [0, 1, 0] and gx.tolist() == [4.0, 18.0, 13.0]


def test_one_entry_of_5000_products(ea, ctx):
    A = (np.array([0, 5000], np.int32), np.arange(5000, dtype=np.int32), np.ones(5000, np.float32))
    B = (np.arange(5001, dtype=np.int32), np.zeros(5000, np.int32), np.ones(5000, np.float32))
    (gp, gj, gx), _, st = check_exact(ea, ctx, A, B, 5000, 1)
    assert gp.tolist() == [0, 1] and gj.tolist() == [0] and gx.tolist() == [5000.0]
    assert st.edges_expanded == 5000


def test_dense_rows_wider_than_lds(ea, ctx):
    A, B = dense_pair()
    (gp, gj, gx), _, st = check_exact(ea, ctx, A, B, 1, 40000)
    assert (np.diff(gp) == 40000).all() and st.vertices_reached == 64
    assert (gj.reshape(64, 40000) == np.arange(40000)).all()


def _identity(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)


def test_identity_and_permutation_times_multigraph(ea, ctx):
    g, B = rmat(ea, ctx, 8)
    n = g.n_rows
    assert len(np.unique(np.repeat(np.arange(n), np.diff(B[0])) * n + B[1])) < g.nnz  # it has repeats
    (lp, lj, lx), _, _ = check_exact(ea, ctx, _identity(n), B, n, n, None, g)
    (rp, rj, rx), _, _ = check_exact(ea, ctx, B, _identity(n), n, n, g, None)
    assert lp.tolist() == rp.tolist() and (lj == rj).all() and (lx == rx).all()
    assert all((np.diff(lj[lp[i]:lp[i + 1]]) > 0).all() for i in range(n))
    assert lx.sum(dtype=np.float64) == B[2].sum(dtype=np.float64)  # weights of repeats add
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    P = (np.arange(n + 1, dtype=np.int32), perm, np.ones(n, np.float32))
    (pp, pj, px), _, _ = check_exact(ea, ctx, P, B, n, n, None, g)
    for i in (0, 1, n // 2, n - 1):  # row i of P * B is row perm[i] of I * B
        k = perm[i]
        assert (pj[pp[i]:pp[i + 1]] == lj[lp[k]:lp[k + 1]]).all() and (px[pp[i]:pp[i + 1]] == lx[lp[k]:lp[k + 1]]).all()


def test_cancelling_products_keep_their_entry(ea, ctx):
    A = csr(2, 3, [(0, 0, 1.0), (0, 1, -1.0), (1, 2, 2.0)])
    B = csr(3, 4, [(0, 3, 1.0), (1, 3, 1.0), (1, 0, 5.0), (2, 2, 1.0)])
    (gp, gj, gx), _, _ = check_exact(ea, ctx, A, B, 3, 4)
    assert gp.tolist() == [0, 2, 3] and gj.tolist() == [0, 3, 2] and gx.tolist() == [-5.0, 0.0, 2.0]


def test_emission_order_against_sorted_rows(ea, ctx):
    g, m = rmat(ea, ctx, 10)
    got, _, _ = rmat10_square(ea, ctx)
    s = g.sorted_rows(ctx)
    assert not (host(s)[1] == m[1]).all()  # the rows were not sorted to begin with
    assert same(arrays(ea, ctx, g, s), got)
    assert same(arrays(ea, ctx, s, s), got)


def test_in_edges_and_hot_first_copy_are_ignored(ea, ctx):
    got, _, _ = rmat10_square(ea, ctx)
    g = ea.Graph.rmat(ctx, 10, 8, 1, 7)
    g.hot_first(ctx, True)
    assert same(arrays(ea, ctx, g, g), got)
    d, m = rmat(ea, ctx, 10, symmetrize=False)
    want = arrays(ea, ctx, d, d)
    e = ea.Graph.rmat(ctx, 10, 8, 1, 7, False)
    e.build_in_edges(ctx)
    assert same(arrays(ea, ctx, e, e), want)
    assert all((x == y).all() for x, y in zip(host(e), m))  # and the operand is what it was


# ---- 3. R-MAT products, exact ----------------------------------------------------------------------

@pytest.mark.parametrize("scale", [8, 10])
def test_rmat_square_with_weights(ea, ctx, scale):
    if scale == 10:
        _, want, _ = rmat10_square(ea, ctx)
    else:
        g, m = rmat(ea, ctx, scale)
        _, want, _ = check_exact(ea, ctx, m, m, g.n_rows, g.n_cols, g, g)
    assert want[4].max() > 2 ** 20  # the sums are large, and still exact


@pytest.mark.parametrize("symmetrize", [True, False])
def test_rmat12_square_unit_weights(ea, ctx, symmetrize):
    g, m = rmat(ea, ctx, 12, 16, 1, 0, symmetrize)
    _, want, st = check_exact(ea, ctx, m, m, g.n_rows, g.n_cols, g, g)
    assert np.diff(want[0]).max() > 2048  # rows of more than a medium table


def test_rmat10_directed_pair(ea, ctx):
    a, A = rmat(ea, ctx, 10, symmetrize=False)
    b, B = rmat(ea, ctx, 10, seed=2, symmetrize=False)
    check_exact(ea, ctx, A, B, a.n_cols, b.n_cols, a, b)


# ---- 4. associativity: the result is an ordinary handle ---------------------------------------------

def test_associativity_and_bfs_on_the_product(ea, ctx, oracle):
    a, m = rmat(ea, ctx, 8, weight_seed=0)
    aa, _ = ea.spgemm(ctx, a, a)
    left = arrays(ea, ctx, aa, a)
    right = arrays(ea, ctx, a, aa)
    assert same(left, right) and left[2].max() < 2 ** 24
    p, j, x = host(aa)
    want = product(*m, *m, a.n_cols)
    assert p.tolist() == want[0].tolist() and (j == want[1]).all()
    depths, _ = ea.bfs(ctx, aa, 0)
    ref, _ = oracle.bfs_heap(p, j, 0)
    assert (depths.cpu().numpy() == ref).all()


# ---- 5. the hooks force the other paths -------------------------------------------------------------

@pytest.mark.parametrize("small", ["0", None])
@pytest.mark.parametrize("slots", ["64", None])
def test_hooks_forced(ea, ctx, monkeypatch, slots, small):
    g, _ = rmat(ea, ctx, 10)
    base, _, _ = rmat10_square(ea, ctx)
    A, B = dense_pair()
    da, db = graph(ea, A, 1), graph(ea, B, 40000)
    dense = arrays(ea, ctx, da, db)
    ka, kb = graph(ea, csr(*KNOWN["A"]), 3), graph(ea, csr(*KNOWN["B"]), 3)
    known = arrays(ea, ctx, ka, kb)
    # and that the hooks are read: there is one launch per populated class and phase, besides the
    # bound and the sum.  Directed R-MAT-12 has rows of the four table classes in both phases (10
    # launches).  64 slots leave the small rows and the dense path in the symbolic phase, where a
    # bound above 32 misses the table, and the wavefront path too in the numeric one (7); without
    # small rows one class fewer per phase (8); both: the wavefront and the dense path (6)
    w, _ = rmat(ea, ctx, 12, 16, 1, 0, False)
    wide = arrays(ea, ctx, w, w)
    assert wide[3].advance_launches == 10
    if slots is not None:
        monkeypatch.setenv(HOOKS[0], slots)
    if small is not None:
        monkeypatch.setenv(HOOKS[1], small)
    assert same(arrays(ea, ctx, g, g), base)
    assert same(arrays(ea, ctx, da, db), dense)
    assert same(arrays(ea, ctx, ka, kb), known)
    forced = arrays(ea, ctx, w, w)
    assert same(forced, wide)
    assert forced[3].advance_launches == {(None, None): 10, ("64", None): 7, (None, "0"): 8, ("64", "0"): 6}[slots, small]


# ---- 6. float weights -------------------------------------------------------------------------------

def test_float_weights_within_the_summation_bound(ea, ctx):
    g, (ap, aj, _) = rmat(ea, ctx, 10)
    ax = np.random.default_rng(11).uniform(-1.0, 1.0, len(aj)).astype(np.float32)
    a = ea.Graph.from_host_csr(ap, aj, ax, g.n_cols)
    cp, cj, cx64, terms, abs_sum, _ = product(ap, aj, ax, ap, aj, ax, g.n_cols)
    gp, gj, gx, _ = arrays(ea, ctx, a, a)
    assert gp.tolist() == cp.tolist() and (gj == cj).all()
    # recursive summation of `terms` float32 products, one rounding per product, doubled
    bound = 2.0 * terms * 2.0 ** -24 * abs_sum
    err = np.abs(gx.astype(np.float64) - cx64)
    print("largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    hp, hj, _, _ = arrays(ea, ctx, a, a)
    assert hp.tolist() == gp.tolist() and (hj == gj).all()


# ---- 7. 64-bit counting -----------------------------------------------------------------------------

def test_products_past_2_to_32(ea, ctx):
    import torch
    A = (np.arange(4097, dtype=np.int32) * 128, np.zeros(4096 * 128, np.int32), np.ones(4096 * 128, np.float32))
    B = (np.array([0, 8192], np.int32), np.arange(8192, dtype=np.int32), np.ones(8192, np.float32))
    c, st = ea.spgemm(ctx, graph(ea, A, 1), graph(ea, B, 8192))
    assert st.edges_expanded == 2 ** 32 and st.edges_traversed == c.nnz == 4096 * 8192
    assert st.vertices_reached == 4096
    cp, cj, cx = (torch.from_numpy(x).cuda() for x in c.to_host())
    assert torch.equal(cp.long(), torch.arange(4097, device="cuda") * 8192)
    assert torch.equal(cj.view(4096, 8192).long(), torch.arange(8192, device="cuda").expand(4096, 8192))
    assert bool((cx == 128.0).all())


def test_result_past_int32_max_is_refused(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    n = 46341  # the smallest n with n * n > INT32_MAX
    A = (np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), np.ones(n, np.float32))
    B = (np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    a, b = graph(ea, A, 1), graph(ea, B, n)
    ea.Context.trim_cache()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(ea.EngineError) as e:
        ea.spgemm(ctx, a, b)
    assert e.value.code == -3 and "2147488281" in str(e.value)
    assert "2147488281" in load_library().grx_last_error().decode()
    after = torch.cuda.mem_get_info()[0]
    # every workspace array of this shape is below 1 MiB (freed, never parked) and the call trims the
    # block cache before it returns: "a few MB" is 8 MiB here; C's arrays would be 16 GiB
    print("device memory before - after the refused call:", before - after, "bytes")
    assert abs(before - after) < 8 << 20
    assert all((x == y).all() for x, y in zip(host(a), A))


# ---- 8. stats ---------------------------------------------------------------------------------------

def test_stats(ea, ctx):
    g, _ = rmat(ea, ctx, 10)
    _, want, st = rmat10_square(ea, ctx)
    cp, cj, _, _, _, products = want
    assert st.edges_expanded == products and st.edges_traversed == len(cj)
    assert st.vertices_reached == int((np.diff(cp) > 0).sum())
    assert st.iterations == 1 and st.advance_launches > 0
    assert st.advance_kernel_ms == 0
    _, timed = ea.spgemm(ctx, g, g, ea.Options(collect_kernel_time=True))
    assert 0 < timed.advance_kernel_ms <= timed.elapsed_ms
    assert timed.edges_expanded == products and timed.advance_launches == st.advance_launches
    assert len(timed.frontier_slots) == 3 and sum(timed.frontier_slots) <= timed.elapsed_ms * 1000 + 3


# ---- 9. argument errors -----------------------------------------------------------------------------

def test_argument_errors(ea, ctx):
    from essentials_amd.api import load_library
    A, B = csr(*KNOWN["A"]), csr(*KNOWN["B"])
    a, b = graph(ea, A, 3), graph(ea, B, 3)
    lib = load_library()
    out = C.c_void_p()
    assert lib.grx_spgemm(ctx._h, a._h, b._h, None, None, None) == -1
    assert lib.grx_spgemm(None, a._h, b._h, C.byref(out), None, None) == -1
    assert lib.grx_spgemm(ctx._h, None, b._h, C.byref(out), None, None) == -1
    assert lib.grx_spgemm(ctx._h, a._h, None, C.byref(out), None, None) == -1
    assert not out.value
    with pytest.raises(ea.EngineError) as e:
        ea.spgemm(ctx, a, graph(ea, csr(4, 3, [(3, 0, 1.0)]), 3))
    assert e.value.code == -1
    with pytest.raises(ea.EngineError) as e:
        ea.spgemm(ctx, a, b, ea.Options(max_iterations=3))
    assert e.value.code == -1
    assert all((x == y).all() for x, y in zip(host(a), A))
    assert all((x == y).all() for x, y in zip(host(b), B))
    c, _ = ea.spgemm(ctx, a, b)  # and the operands still multiply
    assert c.to_host()[2].tolist() == KNOWN["C"][2]


# ---- 10. invariants at RMAT-14 ----------------------------------------------------------------------

def test_rmat14_invariants(ea, ctx):
    import torch
    g = ea.Graph.rmat(ctx, 14, 8, 1, 0)
    s = g.simple(ctx)
    n = s.n_rows
    c, st = ea.spgemm(ctx, s, s)
    assert st.edges_traversed == c.nnz > 10 * s.nnz
    cp, cj, cx = (torch.from_numpy(x).cuda() for x in c.to_host())
    sp, sj, _ = (torch.from_numpy(x).cuda() for x in s.to_host())
    cp, cj, sp, sj = cp.long(), cj.long(), sp.long(), sj.long()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), cp[1:] - cp[:-1])
    keys = rows * n + cj
    assert bool((keys[1:] > keys[:-1]).all())  # every row strictly ascending (and the rows in order)
    assert int((cp[1:] - cp[:-1]).max()) > 2048
    deg = sp[1:] - sp[:-1]

    def lookup(want):
        at = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
        return torch.where(keys[at] == want, cx[at].double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    # C[i, i] = deg_S(i): S is symmetric and simple
    diag = lookup(torch.arange(n, device="cuda") * (n + 1))
    assert torch.equal(diag, deg.double())
    # the entries of C under S: sum over j in row i of S of C[i, j] = 2 * triangles at i
    srows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    under = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, srows, lookup(srows * n + sj))
    tri, _, _ = ea.tc(ctx, s)
    assert torch.equal(under, 2.0 * tri.double())
    # row sums of C = S * deg
    sums = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, rows, cx.double())
    want = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, srows, deg[sj].double())
    assert torch.equal(sums, want)
    c2, _ = ea.spgemm(ctx, s, s)
    for x, y in zip(c.to_host(), c2.to_host()):
        assert torch.equal(torch.from_numpy(x), torch.from_numpy(y))
