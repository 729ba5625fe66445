"""grx_ppr (batched personalized PageRank, 64 seeds to a wavefront) against the float64 oracle of
tests/ppr_oracle.py: bit for bit where float32 is exact, within the derived rounding bound elsewhere,
and bit for bit against its own single-seed calls.  Every call is made twice and must repeat itself.
Each case is named for what can go wrong at its shape."""
import ctypes as C
import os

import numpy as np
import pytest

from ppr_oracle import csr, exact_cases, exact_in_float32, ppr, rounding_bound, transpose

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
CASES = exact_cases()


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ctx, ap, aj, aw, directed=False, n_cols=None):
    g = ea.Graph.from_host_csr(ap, aj, aw, n_cols)
    return g.build_in_edges(ctx) if directed else g


def twice(ea, ctx, g, seeds, alpha, tol, T=0, **kw):
    """Two calls of ea.ppr: the second repeats the first bit for bit.  -> (p, info, Stats) of the first."""
    import torch
    first = None
    for _ in range(2):
        p, info, st = ea.ppr(ctx, g, seeds, alpha=alpha, tol=tol, options=ea.Options(max_iterations=T), **kw)
        count = g.n_rows if seeds is None else len(np.atleast_1d(seeds))
        assert str(p.dtype) == "torch.float32" and tuple(p.shape) == (count, g.n_rows)
        assert info["iterations"].dtype == np.int32 and info["residual"].dtype == np.float32
        assert len(info["iterations"]) == len(info["residual"]) == count
        assert st.edges_traversed == st.edges_expanded == g.nnz * st.iterations
        assert st.vertices_reached == int((p > 0).sum())
        if first is None:
            first = (p.clone(), info, st)
        else:
            assert torch.equal(p, first[0])
            assert (info["iterations"] == first[1]["iterations"]).all()
            assert (info["residual"] == first[1]["residual"]).all()
            assert st.iterations == first[2].iterations and st.frontier_slots == first[2].frontier_slots
            assert st.vertices_reached == first[2].vertices_reached
    return first


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_exact(ea, ctx, g, want, seeds, alpha, tol, T):
    """The call gives the oracle's answer `want` bit for bit, and the stats the answer defines."""
    p, info, st = twice(ea, ctx, g, seeds, alpha, tol, T)
    host = p.cpu().numpy()
    assert (bits(host) == bits(want["p"])).all(), np.abs(host - want["p"]).max()
    assert info["iterations"].tolist() == want["iterations"].tolist()
    assert (bits(info["residual"]) == bits(want["residual"])).all()
    assert st.iterations == want["total"] and st.vertices_reached == want["reached"]
    assert st.frontier_slots == want["active"]  # its length is levels_recorded
    return p, info, st


def exact_case(ea, ctx, name):
    c = CASES[name]
    kw = dict(seeds=c["seeds"], alpha=c["alpha"], tol=c["tol"], max_iterations=c["T"],
              in_edges=transpose(c["ap"], c["aj"], c["aw"]) if c["directed"] else None)
    g = graph(ea, ctx, c["ap"], c["aj"], c["aw"], c["directed"])
    return g, c, ppr(c["ap"], c["aj"], c["aw"], **kw)


# ---- where float32 is exact: the oracle bit for bit ------------------------------------------------

@pytest.mark.parametrize("name", ["ring", "cube"])
def test_exact_on_regular_graphs(ea, ctx, name):
    g, c, want = exact_case(ea, ctx, name)
    check_exact(ea, ctx, g, want, c["seeds"], c["alpha"], c["tol"], c["T"])


@pytest.mark.parametrize("segment", [None, "64"])
def test_exact_on_a_star_whose_hub_row_is_cut(ea, ctx, monkeypatch, segment):
    """An in-row of 4096 entries: 8 partial sums by default, 64 with the hook at its minimum, added in
    segment order; the hub is seed 0's own vertex and a non-seed for seed 7."""
    g, c, want = exact_case(ea, ctx, "star")
    if segment:
        monkeypatch.setenv("GRX_PPR_SEGMENT", segment)
    p, _, _ = check_exact(ea, ctx, g, want, c["seeds"], c["alpha"], c["tol"], c["T"])
    assert p[0, 0] > 0.5 and 0 < p[1, 0] < 0.5


def test_directed_path_returns_dangling_mass_to_the_seed(ea, ctx):
    """In-edges attached; the sink is dangling, and seed 5 is the sink itself: its row stays e_5."""
    g, c, want = exact_case(ea, ctx, "path")
    p, info, _ = check_exact(ea, ctx, g, want, c["seeds"], c["alpha"], c["tol"], c["T"])
    assert p[2].tolist() == [0.0] * 5 + [1.0] and info["residual"][2] == 0
    assert abs(float(p[0].sum()) - 1) == 0 and p[0, 0] > 0.5


def test_directed_k4_uses_the_in_edge_values(ea, ctx):
    """Row weights {2, 1, 1}: the in-row of v holds the 2 of v - 1, which the out-row of v does not."""
    g, c, want = exact_case(ea, ctx, "k4")
    p, _, _ = check_exact(ea, ctx, g, want, c["seeds"], c["alpha"], c["tol"], c["T"])
    wrong = ppr(c["ap"], c["aj"], c["aw"], c["seeds"], alpha=c["alpha"], tol=0, max_iterations=c["T"])
    assert np.abs(wrong["p"] - want["p"]).max() > 1e-3  # the out-rows as in-rows give another answer


# ---- freezing ------------------------------------------------------------------------------------------

def test_a_frozen_column_does_not_change(ea, ctx):
    """Ring of 8 plus an isolated vertex, by tol 2^-8: the isolated seed stops after 1 iteration and is
    carried, frozen, through 6 more; each row is the single-seed call bit for bit."""
    import torch
    g, c, want = exact_case(ea, ctx, "ring_isolated")
    p, info, st = check_exact(ea, ctx, g, want, c["seeds"], c["alpha"], c["tol"], 0)
    assert info["iterations"].tolist() == [7, 1] and st.iterations == 7
    assert p[1].tolist() == [0.0] * 8 + [1.0]
    assert st.frontier_slots == [2, 1, 1, 1, 1, 1, 1]
    for i, s in enumerate(c["seeds"]):
        single, one, _ = twice(ea, ctx, g, [s], c["alpha"], c["tol"])
        assert torch.equal(single[0], p[i]) and one["iterations"][0] == info["iterations"][i]
    both = twice(ea, ctx, g, [8, 0], c["alpha"], c["tol"])  # the other lane order
    assert torch.equal(both[0][0], p[1]) and torch.equal(both[0][1], p[0])


# ---- batch edges ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chesapeake(ea):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, aw = g.to_host()
    assert g.n_rows == 39 and (aw == 1).all()
    return g, ap, ppr(ap, aj, aw, None, alpha=0.85, tol=0, max_iterations=20)


@pytest.mark.parametrize("count", [1, 15, 16, 17, 63, 64, 65, 128])
def test_batch_edges_on_chesapeake(ea, ctx, chesapeake, count):
    """V = 39 is no multiple of any tile; the counts cover every width (16, 32, 64 lanes), lane 63 and a
    second batch of one."""
    import torch
    g, ap, want = chesapeake
    seeds = (np.arange(count) * 7 + 3) % 39  # cycled: vertices repeat inside and across batches
    p, info, st = twice(ea, ctx, g, seeds, 0.85, 0.0, 20)
    bound = rounding_bound(int(np.diff(ap).max()), int((np.diff(ap) == 0).sum()), 0.85)
    host = p.cpu().numpy().astype(np.float64)
    error = np.abs(host - want["p"][seeds]).sum(1)
    print(f"count {count}: largest L1 error {error.max():.3e}, bound {bound:.3e}")
    assert (error <= bound).all()
    assert (np.abs(host.sum(1) - 1) <= bound).all()
    assert info["iterations"].tolist() == [20] * count
    assert st.iterations == 20 * ((count + 63) // 64) and st.frontier_slots == [min(count, 64)] * 20
    for i in range(39, count):
        assert torch.equal(p[i], p[i - 39])


# ---- batch independence on general floats ------------------------------------------------------------

@pytest.fixture(scope="module")
def rmat(ea, ctx):
    """scale -> (graph as generated: a multigraph with loops and integer weights; ap; 65 seeds, the last
    a repeat of the first: two batches, the second of one column; the oracle's T = 20 run)."""
    out = {}
    for scale in (10, 12):
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, aw = g.to_host()
        picked = np.random.default_rng(scale).choice(g.n_rows, 64, replace=False)
        seeds = np.concatenate([picked, picked[:1]]).astype(np.int32)
        out[scale] = (g, ap, seeds, ppr(ap, aj, aw, seeds, alpha=0.85, tol=0, max_iterations=20))
    return out


@pytest.mark.parametrize("scale", [10, 12])
def test_rows_do_not_depend_on_the_batch(ea, ctx, rmat, monkeypatch, scale):
    import torch
    g, ap, seeds, want = rmat[scale]
    degree = np.diff(ap)
    bound = rounding_bound(int(degree.max()), int((degree == 0).sum()), 0.85)
    assert degree.max() > 512 and (degree == 0).any()  # a long in-row and a dangling list
    for tol, T in ((1e-6, 0), (0.0, 20)):
        p, info, st = twice(ea, ctx, g, seeds, 0.85, tol, T)
        for i in (0, 31, 63, 64):
            single, one, _ = twice(ea, ctx, g, [int(seeds[i])], 0.85, tol, T)
            assert torch.equal(single[0], p[i]), i
            assert one["iterations"][0] == info["iterations"][i] and one["residual"][0] == info["residual"][i]
        assert torch.equal(p[64], p[0]) and info["iterations"][64] == info["iterations"][0]
        assert st.iterations == info["iterations"][:64].max() + info["iterations"][64]
        if T:
            error = np.abs(p.cpu().numpy().astype(np.float64) - want["p"]).sum(1)
            print(f"RMAT-{scale}: largest L1 error {error.max():.3e}, bound {bound:.3e}")
            assert (error <= bound).all()
            assert info["iterations"].tolist() == [20] * 65
            with monkeypatch.context() as m:
                m.setenv("GRX_PPR_SEGMENT", "64")
                cut, _, _ = twice(ea, ctx, g, seeds, 0.85, tol, T)
            error = np.abs(cut.cpu().numpy().astype(np.float64) - want["p"]).sum(1)
            print(f"RMAT-{scale}, segments of 64: largest L1 error {error.max():.3e}, bound {bound:.3e}")
            assert (error <= bound).all()
        else:
            # columns freeze at different iterations (an isolated seed after its first)
            assert (info["residual"] < 1e-6).all() and len(set(info["iterations"].tolist())) > 1


# ---- degenerate graphs ---------------------------------------------------------------------------------

def test_one_vertex(ea, ctx):
    for loop in (False, True):
        ap, aj, aw = csr(1, [(0, 0)] if loop else [], symmetric=False)
        g = graph(ea, ctx, ap, aj, aw)
        p, info, st = twice(ea, ctx, g, [0, 0], 0.85, 1e-6)
        assert p.tolist() == [[1.0], [1.0]] and info["iterations"].tolist() == [1, 1]
        assert info["residual"].tolist() == [0.0, 0.0] and st.iterations == 1 and st.vertices_reached == 2


def test_two_vertices(ea, ctx):
    ap, aj, aw = csr(2, [(0, 1)])
    want = ppr(ap, aj, aw, [0, 1], alpha=0.5, tol=0, max_iterations=3)
    p, _, _ = check_exact(ea, ctx, graph(ea, ctx, ap, aj, aw), want, [0, 1], 0.5, 0.0, 3)
    assert p.tolist() == [[0.625, 0.375], [0.375, 0.625]]


def test_no_edges(ea, ctx):
    """Every vertex is dangling: each seed's row is e_s after one iteration."""
    ap, aj, aw = csr(5, [])
    p, info, st = twice(ea, ctx, graph(ea, ctx, ap, aj, aw), None, 0.85, 1e-6)
    assert (p.cpu().numpy() == np.eye(5, dtype=np.float32)).all()
    assert info["iterations"].tolist() == [1] * 5 and st.iterations == 1 and st.vertices_reached == 5


def test_empty_seed_list(ea, ctx):
    ap, aj, aw = csr(3, [(0, 1)])
    p, info, st = ea.ppr(ctx, graph(ea, ctx, ap, aj, aw), [])
    assert tuple(p.shape) == (0, 3) and len(info["iterations"]) == 0 and len(info["residual"]) == 0
    assert st.iterations == 0 and st.advance_launches == 0 and st.elapsed_ms == 0


def test_every_vertex_of_two_triangles(ea, ctx):
    """seeds=None on 7 vertices, one of them isolated: 7 columns in 16 lanes."""
    ap, aj, aw = csr(7, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)])
    assert exact_in_float32(ap, aj, aw, None, alpha=0.5, tol=0, max_iterations=8)
    want = ppr(ap, aj, aw, None, alpha=0.5, tol=0, max_iterations=8)
    p, _, _ = check_exact(ea, ctx, graph(ea, ctx, ap, aj, aw), want, None, 0.5, 0.0, 8)
    assert p[6].tolist() == [0.0] * 6 + [1.0] and float(p[0, 3:].sum()) == 0


def test_a_weight_row_summing_to_zero_is_dangling(ea, ctx):
    """0 -> 1 (+1), 0 -> 2 (-1), 1 -> 0, 2 -> 0: W(0) == 0, so 0 hands nothing on and its mass returns
    to the seed."""
    ap, aj, aw = csr(3, [(0, 1), (0, 2), (1, 0), (2, 0)], weights=[1, -1, 1, 1], symmetric=False)
    kw = dict(alpha=0.5, tol=0, max_iterations=6, in_edges=transpose(ap, aj, aw))
    assert exact_in_float32(ap, aj, aw, [0, 1], **kw)
    want = ppr(ap, aj, aw, [0, 1], **kw)
    assert want["p"][0].tolist() == [1.0, 0.0, 0.0] and want["p"][1][2] == 0
    check_exact(ea, ctx, graph(ea, ctx, ap, aj, aw, directed=True), want, [0, 1], 0.5, 0.0, 6)


# ---- the caller's tensor and the clocks --------------------------------------------------------------

def test_stats_and_a_callers_tensor(ea, ctx, chesapeake):
    import torch
    g, ap, want = chesapeake
    mine = torch.full((39 * 39,), -1.0, dtype=torch.float32, device="cuda")
    out, _, st = ea.ppr(ctx, g, None, tol=0.0, p=mine, options=ea.Options(collect_kernel_time=True, max_iterations=20))
    assert out.data_ptr() == mine.data_ptr() and tuple(out.shape) == (39, 39)
    plain, _, unclocked = ea.ppr(ctx, g, None, tol=0.0, options=ea.Options(max_iterations=20))
    assert torch.equal(out, plain)
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms and st.advance_launches >= 20 * 2
    assert unclocked.advance_kernel_ms == 0 and unclocked.elapsed_ms > 0
    # the mean over all seeds is the global PageRank vector
    ranks, _ = ea.pagerank(ctx, g, 0.85, 1e-6)
    by_tol, _, _ = ea.ppr(ctx, g, None, tol=1e-6)
    assert float((by_tol.mean(0) - ranks).abs().max()) < 5e-5  # each within tol * alpha / (1 - alpha) of the limit
    with pytest.raises(TypeError):
        ea.ppr(ctx, g, None, p=mine.double())
    with pytest.raises(ValueError):
        ea.ppr(ctx, g, None, p=mine[:-1])
    with pytest.raises(ValueError):
        ea.ppr(ctx, g, [[0, 1], [2, 3]])


# ---- errors --------------------------------------------------------------------------------------------

def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    v = np.arange(9)
    ap, aj, aw = csr(10, np.concatenate([np.stack([v, v + 1], 1), [[9, 0], [5, 2]]]), symmetric=False)
    g = graph(ea, ctx, ap, aj, aw)
    g.build_in_edges(ctx)

    def refused(code, **kw):
        with pytest.raises(ea.EngineError) as e:
            ea.ppr(ctx, kw.pop("on", g), **kw)
        assert e.value.code == code and b"grx_ppr" in lib.grx_last_error()

    refused(-1, seeds=[3, -1])
    refused(-1, seeds=[3, 10])
    refused(-1, on=graph(ea, ctx, ap, aj, aw, n_cols=11), seeds=[0])
    refused(-1, seeds=[0], alpha=-0.1)
    refused(-1, seeds=[0], alpha=1.0)
    refused(-1, seeds=[0], alpha=float("nan"))
    refused(-1, seeds=[0], tol=float("nan"))
    refused(-1, seeds=[0], tol=0.0)
    refused(-1, seeds=[0], tol=-1.0)
    refused(-1, seeds=[0], options=ea.Options(max_iterations=-1))
    one = (C.c_int32 * 1)(0)
    out = torch.full((10,), -7.0, dtype=torch.float32, device="cuda")
    args = (0.85, 1e-6, out.data_ptr(), None, None, None, None)
    assert lib.grx_ppr(ctx._h, g._h, one, -1, *args) == -1 and b"grx_ppr" in lib.grx_last_error()
    assert lib.grx_ppr(ctx._h, g._h, None, 1, *args) == -1 and b"grx_ppr" in lib.grx_last_error()
    assert lib.grx_ppr(None, g._h, one, 1, *args) == -1
    assert lib.grx_ppr(ctx._h, None, one, 1, *args) == -1
    assert lib.grx_ppr(ctx._h, g._h, one, 1, 0.85, 1e-6, None, None, None, None, None) == -1
    assert b"d_p" in lib.grx_last_error()
    assert (out == -7).all()
    # ... and the same arguments put right
    assert lib.grx_ppr(ctx._h, g._h, one, 1, *args) == 0
    assert abs(float(out.sum()) - 1) < 1e-5 and out[0] > 0.15


def test_an_asymmetric_csr_needs_in_edges(ea, ctx):
    from essentials_amd.api import load_library
    lib = load_library()
    c = CASES["path"]
    g = graph(ea, ctx, c["ap"], c["aj"], c["aw"])
    with pytest.raises(ea.EngineError) as e:
        ea.ppr(ctx, g, c["seeds"], alpha=0.5)
    assert e.value.code == -3
    message = lib.grx_last_error()
    assert b"grx_ppr" in message and b"grx_graph_build_in_edges" in message
    g.build_in_edges(ctx)
    want = ppr(c["ap"], c["aj"], c["aw"], c["seeds"], alpha=0.5, tol=0, max_iterations=c["T"],
               in_edges=transpose(c["ap"], c["aj"], c["aw"]))
    check_exact(ea, ctx, g, want, c["seeds"], 0.5, 0.0, c["T"])
