"""grx_bfs_multi (multi-source BFS, 64 searches to a word) against the per-source oracle of
tests/bfs_multi_oracle.py and against grx_bfs itself, exactly: depths, the three summaries and the
stats that the answer defines, twice per graph.  Each case is named for what can go wrong at its
shape."""
import ctypes as C
import os

import numpy as np
import pytest

from bfs_multi_oracle import UNREACHED, csr, multi_source

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def graph(ea, ap, aj, n_cols=None):
    return ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols)


def check(ea, ctx, g, want, sources, options=None):
    """Two calls of ea.bfs_multi(g, sources): both give the oracle's answer `want`, bit for bit."""
    import torch
    first = None
    for _ in range(2):
        depths, summary, st = ea.bfs_multi(ctx, g, sources, options=options)
        count = len(want["reached"])
        assert str(depths.dtype) == "torch.int32" and tuple(depths.shape) == (count, g.n_rows)
        host = depths.cpu().numpy()
        print(f"V {g.n_rows} nnz {g.nnz} count {count} iterations {st.iterations} pulls {st.pull_iterations} "
              f"traversed {st.edges_traversed} expanded {st.edges_expanded} launches {st.advance_launches} "
              f"elapsed_ms {st.elapsed_ms:.3f}")
        assert (host == want["depths"]).all()
        assert summary["reached"].dtype == np.int64 and summary["reached"].tolist() == want["reached"].tolist()
        assert summary["depth_sum"].dtype == np.int64 and summary["depth_sum"].tolist() == want["depth_sum"].tolist()
        assert summary["eccentricity"].dtype == np.int32
        assert summary["eccentricity"].tolist() == want["eccentricity"].tolist()
        assert st.iterations == sum(want["levels"])
        assert st.vertices_reached == int(want["reached"].sum())
        assert st.frontier_slots == want["active"][:64]  # its length is levels_recorded
        assert st.edges_traversed == want["traversed"]
        if st.pull_iterations == 0:
            assert st.edges_expanded == st.edges_traversed
        if first is None:
            first = (depths.clone(), summary, st)
        else:
            assert torch.equal(depths, first[0])
            for key in ("reached", "depth_sum", "eccentricity"):
                assert (summary[key] == first[1][key]).all()
            assert st.iterations == first[2].iterations and st.frontier_slots == first[2].frontier_slots
    return first


def forced_pull(ea):
    return ea.Options(direction_optimized=True, do_alpha=1e9)  # every level with an edge pulls


def pulled_levels(want):
    return sum(sum(1 for d in batch if d > 0) for batch in want["degrees"])


# ---- agreement with grx_bfs --------------------------------------------------------------------

@pytest.fixture(scope="module")
def rmat(ea, ctx):
    """scale -> (graph as generated: a multigraph with loops and unsorted rows; ap, aj; 65 sources,
    the last a repeat of the first: two batches, the second of one bit; the oracle's answer)."""
    out = {}
    for scale in (10, 12):
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        ap, aj, _ = g.to_host()
        src = np.repeat(np.arange(g.n_rows), np.diff(ap))
        assert (src == aj).any() and len(np.unique(src.astype(np.int64) * g.n_rows + aj)) < len(aj)
        picked = np.random.default_rng(scale).choice(g.n_rows, 64, replace=False)
        sources = np.concatenate([picked, picked[:1]]).astype(np.int32)
        out[scale] = (g, ap, aj, sources, multi_source(ap, aj, sources))
    return out


@pytest.mark.parametrize("scale", [10, 12])
def test_every_row_is_grx_bfs(ea, ctx, rmat, scale):
    g, ap, aj, sources, want = rmat[scale]
    depths, summary, st = check(ea, ctx, g, want, sources)
    for i, s in enumerate(sources):
        single, _ = ea.bfs(ctx, g, int(s))
        assert (depths[i] == single).all(), (i, s)
    assert (depths[64] == depths[0]).all()
    for key in ("reached", "depth_sum", "eccentricity"):
        assert summary[key][64] == summary[key][0]
    assert len(want["levels"]) == 2


# ---- batch edges -------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 63, 64, 65, 128])
def test_batch_edges_on_chesapeake(ea, ctx, count):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    sources = (np.arange(count) * 7 + 3) % 39  # cycled: vertices repeat inside and across batches
    check(ea, ctx, g, multi_source(ap, aj, sources), sources)


def test_every_bit_carries_its_own_depth(ea, ctx):
    """A path of 64 with all 64 vertices as sources in order: on every vertex the bits 0, 31, 32 and 63
    (the sign bit of a signed word) have distinct depths."""
    n = 64
    v = np.arange(n - 1)
    ap, aj = csr(n, np.stack([v, v + 1], 1))
    sources = np.arange(n)
    depths, summary, _ = check(ea, ctx, graph(ea, ap, aj), multi_source(ap, aj, sources), sources)
    host = depths.cpu().numpy()
    assert (host == np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])).all()
    # ... on every vertex but the two that lie midway between two of them (16: 0 and 32; 47: 31 and 63)
    distinct = [w for w in range(n) if len({int(host[b, w]) for b in (0, 31, 32, 63)}) == 4]
    assert distinct == [w for w in range(n) if w not in (16, 47)]
    assert host[63].tolist() == list(range(63, -1, -1)) and host[31, 63] == 32 and host[32, 0] == 32
    assert summary["eccentricity"][63] == 63 and summary["depth_sum"][63] == 63 * 64 // 2


# ---- a vertex active on many levels ------------------------------------------------------------

def test_a_vertex_active_on_many_levels(ea, ctx):
    """A path of 3000, sources at both ends and the middle: interior vertices enter the active list at
    three different levels, and the search is 3000 levels of one hand-off each."""
    n = 3000
    v = np.arange(n - 1)
    ap, aj = csr(n, np.stack([v, v + 1], 1))
    sources = [0, n - 1, n // 2]
    want = multi_source(ap, aj, sources)
    assert len({int(want["depths"][i, 700]) for i in range(3)}) == 3
    _, _, st = check(ea, ctx, graph(ea, ap, aj), want, sources)
    assert st.iterations == 3000


# ---- one word, many writers ----------------------------------------------------------------------

def _star(leaves=5000):
    leaf = np.arange(1, leaves + 1)
    return csr(leaves + 1, np.stack([np.zeros(leaves, int), leaf], 1))


def test_one_word_many_writers(ea, ctx, monkeypatch):
    """A star with 5000 leaves, 64 of them sources: at level 1 the hub's word takes 64 ORs and is
    listed once; at level 2 its row of 5000 is expanded, by the flat walk or by whole workgroups."""
    import torch
    ap, aj = _star()
    sources = 1 + 78 * np.arange(64)
    want = multi_source(ap, aj, sources)
    g = graph(ea, ap, aj)
    depths, summary, st = check(ea, ctx, g, want, sources)
    assert st.frontier_slots[:3] == [64, 1, 5000]
    for big_row in ("8", "1000000"):  # the leaves' rows flat and the hub's in segments; everything flat
        with monkeypatch.context() as m:
            m.setenv("GRX_BFSM_BIG_ROW", big_row)
            again, summary2, st2 = check(ea, ctx, g, want, sources)
        assert torch.equal(again, depths) and st2.frontier_slots == st.frontier_slots
        assert all((summary2[key] == summary[key]).all() for key in summary)


# ---- unreached and degenerate --------------------------------------------------------------------

def test_unreached_vertices(ea, ctx):
    """Two components plus isolated vertices."""
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1), (10, 11), (11, 12), (11, 12)]
    ap, aj = csr(20, edges)
    sources = [0, 12, 5, 19, 2]
    depths, summary, _ = check(ea, ctx, graph(ea, ap, aj), multi_source(ap, aj, sources), sources)
    host = depths.cpu().numpy()
    assert (host[0, 4:] == UNREACHED).all() and (host[2] == UNREACHED).sum() == 19
    assert summary["reached"].tolist() == [4, 3, 1, 1, 4] and summary["eccentricity"].tolist() == [2, 2, 0, 0, 2]


def test_degenerate_graphs(ea, ctx):
    one = graph(ea, np.zeros(2, np.int32), np.zeros(0, np.int32))
    depths, summary, st = check(ea, ctx, one, multi_source([0, 0], [], [0]), [0])
    assert depths.cpu().tolist() == [[0]] and summary["reached"].tolist() == [1] and st.iterations == 1
    bare = graph(ea, np.zeros(101, np.int32), np.zeros(0, np.int32))
    sources = [5, 7, 5]
    depths, summary, st = check(ea, ctx, bare, multi_source(np.zeros(101, np.int32), [], sources), sources)
    assert int((depths != UNREACHED).sum()) == 3 and st.frontier_slots == [2] and st.advance_launches > 0
    # no vertex, and no source: nothing is written and nothing is launched
    empty = graph(ea, np.zeros(1, np.int32), np.zeros(0, np.int32))
    depths, summary, st = ea.bfs_multi(ctx, empty)
    assert tuple(depths.shape) == (0, 0) and len(summary["reached"]) == 0
    assert st.iterations == 0 and st.advance_launches == 0
    depths, summary, st = ea.bfs_multi(ctx, bare, sources=[])
    assert tuple(depths.shape) == (0, 100) and len(summary["eccentricity"]) == 0
    assert st.iterations == 0 and st.advance_launches == 0 and st.vertices_reached == 0
    from essentials_amd.api import load_library
    ecc = (C.c_int32 * 1)(-7)
    nothing = (C.c_int32 * 1)(0)
    assert load_library().grx_bfs_multi(ctx._h, bare._h, nothing, 0, None, None, None, ecc, None, None) == 0
    assert ecc[0] == -7


def test_every_vertex_of_chesapeake(ea, ctx):
    g = ea.Graph.from_mtx(CHESAPEAKE)
    ap, aj, _ = g.to_host()
    depths, _, _ = check(ea, ctx, g, multi_source(ap, aj), None)
    assert tuple(depths.shape) == (39, 39)
    for i in range(39):
        single, _ = ea.bfs(ctx, g, i)
        assert (depths[i] == single).all()


# ---- directed, and pulling ------------------------------------------------------------------------

def _directed_path_with_a_back_edge(n=200):
    v = np.arange(n - 1)
    return csr(n, np.concatenate([np.stack([v, v + 1], 1), [(n - 1, n // 2)]]), symmetric=False)


def _random_directed(n=500, m=1500):
    return csr(n, np.random.default_rng(3).integers(0, n, size=(m, 2)), symmetric=False)


@pytest.mark.parametrize("shape", [_directed_path_with_a_back_edge, _random_directed])
def test_directed(ea, ctx, shape):
    import torch
    ap, aj = shape()
    n = len(ap) - 1
    sources = np.random.default_rng(8).integers(0, n, 70)
    want = multi_source(ap, aj, sources)
    g = graph(ea, ap, aj)
    depths, _, st = check(ea, ctx, g, want, sources)  # the bare handle: out-entries, pushed
    assert st.pull_iterations == 0
    g.build_in_edges(ctx)
    pushed, _, st = check(ea, ctx, g, want, sources, ea.Options(direction_optimized=False))
    assert st.pull_iterations == 0 and torch.equal(pushed, depths)
    pulled, _, st = check(ea, ctx, g, want, sources, forced_pull(ea))
    assert torch.equal(pulled, depths)
    # every level pulls but those whose active vertices have no out-entry
    assert st.pull_iterations > 0 and st.pull_iterations == pulled_levels(want) <= st.iterations


def test_forced_pull_on_symmetric_rmat(ea, ctx, rmat):
    import torch
    g, ap, aj, sources, want = rmat[10]
    pushed, _, _ = ea.bfs_multi(ctx, g, sources)
    pulled, _, st = check(ea, ctx, g, want, sources, forced_pull(ea))
    assert torch.equal(pulled, pushed) and st.pull_iterations == pulled_levels(want) > 0


def test_forced_pull_of_a_long_in_row(ea, ctx, monkeypatch):
    ap, aj = _star()
    sources = 1 + 78 * np.arange(64)
    want = multi_source(ap, aj, sources)
    g = graph(ea, ap, aj)
    with monkeypatch.context() as m:
        m.setenv("GRX_BFSM_BIG_ROW", "8")
        _, _, st = check(ea, ctx, g, want, sources, forced_pull(ea))
    assert st.pull_iterations == pulled_levels(want) == 3
    with monkeypatch.context() as m:
        m.setenv("GRX_BFSM_BIG_ROW", "1000000")  # the same row in the flat walk
        _, _, st = check(ea, ctx, g, want, sources, forced_pull(ea))
    assert st.pull_iterations == 3


def test_a_long_in_row_gathers_only_what_its_neighbours_have(ea, ctx, monkeypatch):
    """The star plus 40 isolated vertices; bits 0..31 are leaves, bits 32..63 isolated vertices: the
    hub's word, OR-reduced over a workgroup, has bit 31 and must have none of the upper half."""
    leaves = 5000
    ap, aj = csr(leaves + 41, np.stack([np.zeros(leaves, int), np.arange(1, leaves + 1)], 1))
    sources = np.concatenate([1 + 150 * np.arange(32), leaves + 1 + np.arange(32)])
    want = multi_source(ap, aj, sources)
    assert want["reached"].tolist() == [leaves + 1] * 32 + [1] * 32
    g = graph(ea, ap, aj)
    for big_row in ("8", "1000000"):
        with monkeypatch.context() as m:
            m.setenv("GRX_BFSM_BIG_ROW", big_row)
            check(ea, ctx, g, want, sources, forced_pull(ea))
            check(ea, ctx, g, want, sources)


def test_default_alpha_gives_the_same_answer(ea, ctx, rmat):
    g, ap, aj, sources, want = rmat[12]
    _, _, st = check(ea, ctx, g, want, sources, ea.Options(direction_optimized=True))
    print(f"default do_alpha on RMAT-12: {st.pull_iterations} of {st.iterations} levels pulled")


# ---- summaries only --------------------------------------------------------------------------------

def test_summaries_only(ea, ctx, rmat):
    g, ap, aj, sources, want = rmat[10]
    for options in (None, forced_pull(ea)):
        depths, summary, st = ea.bfs_multi(ctx, g, sources, want_depths=False, options=options)
        assert depths is None
        for key in ("reached", "depth_sum", "eccentricity"):
            assert summary[key].tolist() == want[key].tolist()
        assert st.iterations == sum(want["levels"]) and st.vertices_reached == int(want["reached"].sum())


def test_stats_and_a_callers_tensor(ea, ctx, rmat):
    import torch
    g, ap, aj, sources, want = rmat[10]
    mine = torch.full((65 * g.n_rows,), -1, dtype=torch.int32, device="cuda")
    out, _, st = ea.bfs_multi(ctx, g, sources, depths=mine, options=ea.Options(collect_kernel_time=True))
    assert out.data_ptr() == mine.data_ptr() and (out.cpu().numpy() == want["depths"]).all()
    assert 0 < st.advance_kernel_ms <= st.elapsed_ms and st.advance_launches > 0
    _, _, plain = ea.bfs_multi(ctx, g, sources)
    assert plain.advance_kernel_ms == 0 and plain.elapsed_ms > 0
    with pytest.raises(TypeError):
        ea.bfs_multi(ctx, g, sources, depths=mine.long())
    with pytest.raises(ValueError):
        ea.bfs_multi(ctx, g, sources, depths=mine[:-1])


# ---- errors ----------------------------------------------------------------------------------------

def test_argument_errors(ea, ctx):
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj = _directed_path_with_a_back_edge(10)
    g = graph(ea, ap, aj)

    def refused(code, **kw):
        with pytest.raises(ea.EngineError) as e:
            ea.bfs_multi(ctx, kw.pop("on", g), **kw)
        assert e.value.code == code and b"grx_bfs_multi" in lib.grx_last_error()

    refused(-1, sources=[3, -1])
    refused(-1, sources=[3, 10])
    refused(-1, on=graph(ea, ap, aj, n_cols=11), sources=[0])
    refused(-1, sources=[0], options=ea.Options(max_iterations=1))
    # asymmetric and no in-edges: a pull cannot walk backwards (what grx_bfs returns)
    refused(-3, sources=[0], options=ea.Options(direction_optimized=True))
    with pytest.raises(ea.EngineError) as e:
        ea.bfs(ctx, g, 0, options=ea.Options(direction_optimized=True))
    assert e.value.code == -3
    one = (C.c_int32 * 1)(0)
    reached = (C.c_int64 * 1)(-7)
    assert lib.grx_bfs_multi(ctx._h, g._h, one, -1, None, reached, None, None, None, None) == -1
    assert b"grx_bfs_multi" in lib.grx_last_error()
    assert lib.grx_bfs_multi(ctx._h, g._h, one, 1, None, None, None, None, None, None) == -1
    assert b"grx_bfs_multi" in lib.grx_last_error()
    assert lib.grx_bfs_multi(ctx._h, g._h, None, 1, None, reached, None, None, None, None) == -1
    assert lib.grx_bfs_multi(None, g._h, one, 1, None, reached, None, None, None, None) == -1
    assert reached[0] == -7
    # ... and the same arguments put right
    assert lib.grx_bfs_multi(ctx._h, g._h, one, 1, None, reached, None, None, None, None) == 0
    assert reached[0] == 10
