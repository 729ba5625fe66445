"""grx_bfs_predecessors and grx_sssp_predecessors (one pass over the entries, pulled over in-rows by
16-lane groups or pushed over out-rows with an atomic minimum; hops by pointer doubling) against the
numpy oracle, exactly: every output is an integer.  Every call is made twice into tensors filled with
different junk and must repeat itself bit for bit.  Each case is named for what can go wrong there."""
import ctypes as C

import numpy as np
import pytest

from tree_oracle import (FLT_UNREACHED, INT_UNREACHED, SWEEP_LENGTHS, csr, doubling_rounds, entries, sweep_ladder,
                         transpose, tree)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

HOOKS = [None, ("GRX_TREE_PULL", "0"), ("GRX_TREE_SEGMENT", "64")]
HOOK_IDS = ["default", "push", "segment64"]


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


def device(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def twice(ea, ctx, g, source, labels, hops=False, want=None):
    """Two calls of ea.predecessors into tensors filled with something else: the second repeats the
    first bit for bit.  With `want` (the oracle's dict) every output and figure must equal it.
    -> (pred, hops or None as numpy arrays, info, Stats) of the first."""
    import torch
    first = None
    for junk in (7, -9):
        pred = torch.full((g.n_rows,), junk, dtype=torch.int32, device="cuda")
        steps = torch.full((g.n_rows,), junk - 100, dtype=torch.int32, device="cuda") if hops else False
        p, h, info, st = ea.predecessors(ctx, g, source, labels, predecessors=pred, hops=steps)
        assert p.data_ptr() == pred.data_ptr() and (h is None) == (not hops)
        assert st.edges_traversed == st.edges_expanded == g.nnz and st.elapsed_ms > 0 and st.advance_launches >= 1
        got = (p.cpu().numpy(), h.cpu().numpy() if hops else None, info, st)
        if first is None:
            first = got
            continue
        assert (got[0] == first[0]).all() and info == first[2]
        assert not hops or (got[1] == first[1]).all()
        for name in ("iterations", "advance_launches", "vertices_reached", "pull_iterations"):
            assert getattr(st, name) == getattr(first[3], name)
    pred, steps, info, st = first
    if want is not None:
        assert (pred == want["pred"]).all(), np.flatnonzero(pred != want["pred"])[:10]
        assert info == {"orphans": want["orphans"], "violations": want["violations"]}
        assert st.vertices_reached == want["reached"]
        if hops:
            assert (steps == want["hops"]).all(), np.flatnonzero(steps != want["hops"])[:10]
            assert st.iterations == doubling_rounds(want["pred"])
        else:
            assert st.iterations == 0
    return first


class Case:
    """A graph, its host arrays, a source, the labels of both searches from it and the oracle's trees."""

    def __init__(self, ea, ctx, g, source=None):
        self.g = g
        self.ap, self.aj, self.aw = g.to_host()
        self.source = int(np.argmax(np.diff(self.ap))) if source is None else source  # the largest row
        self.labels = {"bfs": ea.bfs(ctx, g, self.source)[0], "sssp": ea.sssp(ctx, g, self.source)[0]}
        self.host = {k: v.cpu().numpy() for k, v in self.labels.items()}
        self.want = {k: tree(self.ap, self.aj, self.aw, v, self.source) for k, v in self.host.items()}


@pytest.fixture(scope="module")
def symmetric(ea, ctx):
    return Case(ea, ctx, ea.Graph.rmat(ctx, 10, 16, 1, 7))


# ---- 1. symmetric R-MAT: the pull form, the push form and short segments agree with the oracle ---------

@pytest.mark.parametrize("hook", HOOKS, ids=HOOK_IDS)
@pytest.mark.parametrize("kind", ["bfs", "sssp"])
def test_symmetric_rmat(ea, ctx, symmetric, monkeypatch, kind, hook):
    """2**10 vertices, hub rows of about 2000 entries (4 items by default, about 32 under the hook),
    empty rows, several sweeps of a workgroup's 16 rows."""
    c = symmetric
    degree = np.diff(c.ap)
    assert degree.max() > 1024 and (degree == 0).any() and degree[c.source] == degree.max()
    if hook:
        monkeypatch.setenv(*hook)
    want = c.want[kind]
    assert want["orphans"] == want["violations"] == 0 and 1 < want["reached"] < c.g.n_rows
    _, _, _, st = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp", want=want)
    assert st.pull_iterations == (0 if hook == HOOKS[1] else 1)
    # pull: the plan, the short rows, the items, the long rows; push: a fill and a pass over all vertices;
    # hops: a begin, an end, and batches of four rounds and a hand-off up to the first round that moves nothing
    hops_launches = 0 if kind == "bfs" else 2 + 5 * ((st.iterations + 1 + 3) // 4)
    assert st.advance_launches - hops_launches == (5 if hook == HOOKS[1] else 4)


# ---- 2. directed R-MAT: pushed without in-edges, pulled with them --------------------------------------

def test_directed_rmat_pushes_then_pulls(ea, ctx, monkeypatch):
    c = Case(ea, ctx, ea.Graph.rmat(ctx, 10, 16, 1, 7, symmetrize=False))
    assert c.want["bfs"]["violations"] == c.want["sssp"]["violations"] == 0
    assert c.want["bfs"]["orphans"] == c.want["sssp"]["orphans"] == 0 and c.want["bfs"]["reached"] > 100
    for kind in ("bfs", "sssp"):
        _, _, _, st = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp", want=c.want[kind])
        assert st.pull_iterations == 0
    c.g.build_in_edges(ctx)
    for segment in (None, "64"):
        if segment:
            monkeypatch.setenv("GRX_TREE_SEGMENT", segment)
        for kind in ("bfs", "sssp"):
            _, _, _, st = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp", want=c.want[kind])
            assert st.pull_iterations == 1


# ---- 3. the smallest id, not the first one ---------------------------------------------------------------

IN_DEGREES = [5000, 15, 16, 17, 63, 64, 65, 511, 512, 513]


def shuffled_fan():
    """Source 0, 5000 vertices at depth 1, and one vertex at depth 2 per entry of IN_DEGREES with that
    many parents; undirected, every row shuffled so that its smallest id is neither first nor last."""
    rng = np.random.default_rng(17)
    middle = 1 + rng.permutation(5000)
    pairs = [(0, int(p)) for p in middle]
    for i, d in enumerate(IN_DEGREES):
        pairs += [(int(p), 5001 + i) for p in rng.permutation(middle)[:d]]
    n = 5001 + len(IN_DEGREES)
    ap, aj, aw = csr(n, pairs)
    for v in range(n):
        row = aj[ap[v]:ap[v + 1]]
        rng.shuffle(row)
        if len(row) > 2:
            at = int(np.argmin(row))
            row[[at, len(row) // 2]] = row[[len(row) // 2, at]]
            assert row.min() not in (row[0], row[-1])
    return n, ap, aj, aw


@pytest.mark.parametrize("hook", HOOKS, ids=HOOK_IDS)
def test_smallest_parent_on_shuffled_rows(ea, ctx, monkeypatch, hook):
    """Every parent of a depth-2 vertex qualifies (unit weights): "the first qualifying entry" instead
    of the minimum, a group's tail lanes and the items of a cut row all show here."""
    import torch
    n, ap, aj, aw = shuffled_fan()
    depths = np.array([0] + [1] * 5000 + [2] * len(IN_DEGREES), np.int32)
    labels = {"bfs": device(depths), "sssp": device(depths.astype(np.float32))}
    want = {k: tree(ap, aj, aw, v.cpu().numpy(), 0) for k, v in labels.items()}
    for i, d in enumerate(IN_DEGREES):
        row = aj[ap[5001 + i]:ap[5002 + i]]
        assert len(row) == d and want["bfs"]["pred"][5001 + i] == row.min() == want["sssp"]["pred"][5001 + i]
    plain = ea.Graph.from_host_csr(ap, aj, aw)
    vouched = ea.Graph.from_host_csr(ap, aj, aw)
    ea.spmv(ctx, vouched, torch.ones(n, dtype=torch.float32, device="cuda"), transpose=True)  # leaves the verdict
    directed = ea.Graph.from_host_csr(ap, aj, aw).build_in_edges(ctx)
    if hook:
        monkeypatch.setenv(*hook)
    pushed = hook == HOOKS[1]
    # who pulls: nobody has vouched for `plain`; a structural verdict is enough for BFS, not for SSSP
    for g, pulls in ((plain, {"bfs": 0, "sssp": 0}), (vouched, {"bfs": 1, "sssp": 0}), (directed, {"bfs": 1, "sssp": 1})):
        for kind in ("bfs", "sssp"):
            _, _, _, st = twice(ea, ctx, g, 0, labels[kind], hops=kind == "sssp", want=want[kind])
            assert st.pull_iterations == (0 if pushed else pulls[kind])


# ---- 4. a valid tree, judged from the outputs alone ------------------------------------------------------

@pytest.mark.parametrize("kind", ["bfs", "sssp"])
def test_the_outputs_are_a_shortest_path_tree(ea, ctx, symmetric, kind):
    c = symmetric
    label = c.host[kind]
    pred, hops, _, _ = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp")
    unreached = INT_UNREACHED if kind == "bfs" else FLT_UNREACHED
    assert pred[c.source] == c.source and ((pred == -1) == (label == unreached)).all() and (pred != -2).all()
    for v in np.flatnonzero((label != unreached) & (np.arange(len(label)) != c.source)):
        u = pred[v]
        row = slice(c.ap[u], c.ap[u + 1])
        weights = c.aw[row][c.aj[row] == v]
        assert len(weights), (u, v)  # the entry (pred[v], v, w) exists
        if kind == "bfs":
            assert label[u] + 1 == label[v]
        else:
            assert ((label[u] + weights.astype(np.float32)) == label[v]).any() and label[u] < label[v]
            walked, x = 0, v
            while x != c.source:
                x, walked = pred[x], walked + 1
                assert walked <= len(label)
            assert walked == hops[v]


def test_hops_on_unit_weights_are_the_depths(ea, ctx, symmetric):
    c = symmetric
    unit = ea.Graph.from_host_csr(c.ap, c.aj, np.ones(len(c.aj), np.float32))
    depths = c.host["bfs"]
    as_float = np.where(depths == INT_UNREACHED, FLT_UNREACHED, depths).astype(np.float32)
    pred, hops, info, _ = twice(ea, ctx, unit, c.source, device(as_float), hops=True)
    assert (hops == np.where(depths == INT_UNREACHED, -1, depths)).all()
    assert (pred == c.want["bfs"]["pred"]).all() and info == {"orphans": 0, "violations": 0}


# ---- 5. doubling over a long chain -----------------------------------------------------------------------

@pytest.mark.parametrize("in_edges", [False, True], ids=["push", "pull"])
def test_doubling_on_a_permuted_path(ea, ctx, in_edges):
    """5000 vertices in a row under a random numbering: neighbours on the path sit in different
    workgroups, and 4999 steps take ceil(log2(4999)) = 13 rounds."""
    order = np.random.default_rng(23).permutation(5000)
    ap, aj, aw = csr(5000, list(zip(order[:-1], order[1:])), symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    if in_edges:
        g.build_in_edges(ctx)
    dist = np.empty(5000, np.float32)
    dist[order] = np.arange(5000)
    source = int(order[0])
    want = tree(ap, aj, aw, dist, source)
    pred, hops, _, st = twice(ea, ctx, g, source, device(dist), hops=True, want=want)
    assert (hops[order] == np.arange(5000)).all() and (pred[order[1:]] == order[:-1]).all()
    assert st.iterations == 13 and st.pull_iterations == int(in_edges)
    assert ea.path(pred, int(order[-1])) == order.tolist()
    assert ea.path(device(pred), int(order[2])) == order[:3].tolist()


# ---- 6. orphans --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("light", [0.0, 2.0 ** -30], ids=["zero", "absorbed"])
@pytest.mark.parametrize("in_edges", [False, True], ids=["push", "pull"])
def test_an_orphan_behind_a_weight_that_adds_nothing(ea, ctx, light, in_edges):
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)], weights=[1.0, light, 1.0], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    if in_edges:
        g.build_in_edges(ctx)
    dist = ea.sssp(ctx, g, 0)[0]
    assert dist.tolist() == [0.0, 1.0, 1.0, 2.0]
    pred, hops, info, st = twice(ea, ctx, g, 0, dist, hops=True, want=tree(ap, aj, aw, dist.cpu().numpy(), 0))
    assert pred.tolist() == [0, 0, -2, 2] and hops.tolist() == [0, 1, -1, -1]
    assert info == {"orphans": 1, "violations": 0} and st.vertices_reached == 4 and st.iterations == 0
    assert ea.path(pred, 3) == [] and ea.path(pred, 1) == [0, 1]


# ---- 7. labels that are no fixed point ---------------------------------------------------------------------

@pytest.mark.parametrize("hook", HOOKS[:2], ids=HOOK_IDS[:2])
def test_violations_of_spoilt_depths(ea, ctx, symmetric, monkeypatch, hook):
    c = symmetric
    depths = c.host["bfs"].copy()
    tree_pred = c.want["bfs"]["pred"]
    reached = np.flatnonzero(depths != INT_UNREACHED)
    leaves = np.setdiff1d(reached[depths[reached] >= 2], tree_pred)  # nobody's predecessor
    leaf = int(leaves[0])
    other = int(np.setdiff1d(reached[depths[reached] == 2], [leaf])[-1])
    depths[leaf] += 2
    depths[other] -= 1
    want = tree(c.ap, c.aj, c.aw, depths, c.source)
    assert want["violations"] > 0
    if hook:
        monkeypatch.setenv(*hook)
    twice(ea, ctx, c.g, c.source, device(depths), want=want)


@pytest.mark.parametrize("hook", HOOKS[:2], ids=HOOK_IDS[:2])
def test_violations_of_a_search_cut_short(ea, ctx, symmetric, monkeypatch, hook):
    c = symmetric
    dist = ea.sssp(ctx, c.g, c.source, options=ea.Options(max_iterations=2))[0]
    want = tree(c.ap, c.aj, c.aw, dist.cpu().numpy(), c.source)
    assert want["violations"] > 0
    if hook:
        monkeypatch.setenv(*hook)
    _, _, info, _ = twice(ea, ctx, c.g, c.source, dist, hops=True, want=want)
    assert info["violations"] == want["violations"] > 0


# ---- 8. shapes ---------------------------------------------------------------------------------------------

def test_one_vertex(ea, ctx):
    g = ea.Graph.from_host_csr(np.zeros(2, np.int32), [], [])
    for labels in (device(np.zeros(1, np.int32)), device(np.zeros(1, np.float32))):
        weighted = labels.dtype.is_floating_point
        pred, hops, info, st = twice(ea, ctx, g, 0, labels, hops=weighted)
        assert pred.tolist() == [0] and info == {"orphans": 0, "violations": 0} and st.vertices_reached == 1
        assert not weighted or (hops.tolist() == [0] and st.iterations == 0)


@pytest.mark.parametrize("in_edges", [False, True], ids=["push", "pull"])
def test_a_source_with_an_empty_row(ea, ctx, in_edges):
    ap, aj, aw = csr(3, [(1, 2)], symmetric=False)
    g = ea.Graph.from_host_csr(ap, aj, aw)
    if in_edges:
        g.build_in_edges(ctx)
    for kind, labels in (("bfs", ea.bfs(ctx, g, 0)[0]), ("sssp", ea.sssp(ctx, g, 0)[0])):
        pred, hops, info, st = twice(ea, ctx, g, 0, labels, hops=kind == "sssp",
                                     want=tree(ap, aj, aw, labels.cpu().numpy(), 0))
        assert pred.tolist() == [0, -1, -1] and st.vertices_reached == 1
        assert hops is None or hops.tolist() == [0, -1, -1]


@pytest.mark.parametrize("in_edges", [False, True], ids=["push", "pull"])
def test_two_components(ea, ctx, in_edges):
    ap, aj, aw = csr(5, [(0, 1), (1, 2), (3, 4)], weights=[2.0, 3.0, 4.0])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    if in_edges:
        g.build_in_edges(ctx)
    for kind, labels in (("bfs", ea.bfs(ctx, g, 0)[0]), ("sssp", ea.sssp(ctx, g, 0)[0])):
        pred, hops, info, st = twice(ea, ctx, g, 0, labels, hops=kind == "sssp",
                                     want=tree(ap, aj, aw, labels.cpu().numpy(), 0))
        assert pred.tolist() == [0, 0, 1, -1, -1] and st.vertices_reached == 3
        assert hops is None or hops.tolist() == [0, 1, 2, -1, -1]
        assert info == {"orphans": 0, "violations": 0}


def test_no_vertices(ea, ctx):
    import torch
    g = ea.Graph.from_host_csr(np.zeros(1, np.int32), [], [])
    for dtype in (torch.int32, torch.float32):
        pred, hops, info, st = ea.predecessors(ctx, g, 0, torch.empty(0, dtype=dtype, device="cuda"))
        assert pred.numel() == 0 and hops is None and info == {"orphans": 0, "violations": 0}
        assert st.advance_launches == 0 and st.elapsed_ms == 0 and st.vertices_reached == 0


# ---- 9. errors ---------------------------------------------------------------------------------------------

def test_argument_errors(ea, ctx):
    import torch
    from essentials_amd.api import load_library
    lib = load_library()
    ap, aj, aw = csr(4, [(0, 1), (1, 2), (2, 3)])
    g = ea.Graph.from_host_csr(ap, aj, aw)
    wide = ea.Graph.from_host_csr(ap, aj, aw, n_cols=6)
    depths, dist = device(np.array([0, 1, 2, 3], np.int32)), device(np.array([0, 1, 2, 3], np.float32))
    pred = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    hops = torch.full((4,), 78, dtype=torch.int32, device="cuda")
    orphans, violations = C.c_int64(-5), C.c_int64(-5)
    cut = ea.Options(max_iterations=3)._c()
    torch.cuda.synchronize()  # the calls below go past the wrapper that orders the engine after torch

    def bfs(c=ctx._h, h=g._h, source=0, labels=depths.data_ptr(), p=pred.data_ptr(), o=C.byref(orphans),
            v=C.byref(violations), opt=None):
        return lib.grx_bfs_predecessors(c, h, source, labels, p, o, v, opt, None)

    def sssp(c=ctx._h, h=g._h, source=0, labels=dist.data_ptr(), p=pred.data_ptr(), hp=hops.data_ptr(),
             o=C.byref(orphans), v=C.byref(violations), opt=None):
        return lib.grx_sssp_predecessors(c, h, source, labels, p, hp, o, v, opt, None)

    for call, name in ((bfs, b"grx_bfs_predecessors"), (sssp, b"grx_sssp_predecessors")):
        for source in (-1, 4):
            assert call(source=source) == -1 and name in lib.grx_last_error() and b"source" in lib.grx_last_error()
        assert call(source=1) == -1 and name in lib.grx_last_error() and b"label[source]" in lib.grx_last_error()
        assert call(h=wide._h) == -1 and name in lib.grx_last_error() and b"square" in lib.grx_last_error()
        assert call(opt=C.byref(cut)) == -1 and name in lib.grx_last_error() and b"max_iterations" in lib.grx_last_error()
        assert call(c=None) == -1 and call(h=None) == -1 and call(labels=None) == -1
        assert name in lib.grx_last_error()
    assert bfs(p=None, o=None, v=None) == -1 and b"output" in lib.grx_last_error()
    assert sssp(p=None, hp=None, o=None, v=None) == -1 and b"output" in lib.grx_last_error()
    ctx.synchronize()
    assert (pred == 77).all() and (hops == 78).all() and orphans.value == violations.value == -5  # nothing ran
    # any one output is enough, and predecessors may be left out
    assert bfs(p=None, o=None) == 0 and violations.value == 0 and orphans.value == -5
    assert sssp(p=None, o=None, v=None) == 0
    ctx.synchronize()
    assert hops.tolist() == [0, 1, 2, 3] and (pred == 77).all()
    assert sssp(hp=None) == 0 and orphans.value == 0
    ctx.synchronize()
    assert pred.tolist() == [0, 0, 1, 2] and hops.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        ea.predecessors(ctx, g, 0, depths, hops=True)
    with pytest.raises(TypeError):
        ea.predecessors(ctx, g, 0, dist.double())
    with pytest.raises(ValueError):
        ea.predecessors(ctx, g, 0, dist[:3])
    with pytest.raises(ea.EngineError) as e:
        ea.predecessors(ctx, g, 2, dist)
    assert e.value.code == -1


# ---- 10. the traversals run on the hot-first copy, the tree call on the caller's CSR -------------------------

def test_labels_of_the_hot_first_copy_in_the_callers_numbering(ea, ctx):
    """2**16 vertices and about 2**21 entries: grx_bfs and grx_sssp renumber, and deliver their labels
    in the caller's numbering; the tree is in that numbering too."""
    c = Case(ea, ctx, ea.Graph.rmat(ctx, 16, 16, 1, 7))
    assert c.g.n_rows >= 2 ** 16 and c.g.nnz >= 2 ** 20  # the size rule of the renumbered copy
    for kind in ("bfs", "sssp"):
        want = c.want[kind]
        assert want["orphans"] == want["violations"] == 0
        _, _, _, st = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp", want=want)
        assert st.pull_iterations == 1
    u, v, qualifies, _ = entries(c.ap, c.aj, c.aw, c.host["sssp"])
    assert qualifies.sum() >= c.want["sssp"]["reached"] - 1


# ---- 11. the edges of the row sweep at one tiny shape --------------------------------------------------------

@pytest.fixture(scope="module")
def ladder(ea, ctx):
    ap, aj, aw = sweep_ladder()
    for offsets in (ap, transpose(ap, aj, aw)[0]):
        assert len(offsets) == 38 and set(SWEEP_LENGTHS) <= set(np.diff(offsets).tolist())
    c = Case(ea, ctx, ea.Graph.from_host_csr(ap, aj, aw), source=10)  # the labels of the graph as given
    c.g.build_in_edges(ctx)
    return c


@pytest.mark.parametrize("segment", [None, "64"])
@pytest.mark.parametrize("pull", [True, False], ids=["pull", "push"])
@pytest.mark.parametrize("kind", ["bfs", "sssp"])
def test_sweep_ladder(ea, ctx, ladder, monkeypatch, kind, pull, segment):
    """37 vertices, in-rows pulled and out-rows pushed: the last sweep of a workgroup has lane groups
    past the end, and under the hook a row of 64 is short, 65 leaves an item of one entry and 200 a
    partial last item.  Vertex 9 has no in-entry: unreached, and its 129 out-entries are items that
    the push form must skip."""
    c = ladder
    want = c.want[kind]
    assert want["pred"][9] == -1 and want["violations"] == 0 and 20 < want["reached"] < 37
    if not pull:
        monkeypatch.setenv("GRX_TREE_PULL", "0")
    if segment:
        monkeypatch.setenv("GRX_TREE_SEGMENT", segment)
    _, _, _, st = twice(ea, ctx, c.g, c.source, c.labels[kind], hops=kind == "sssp", want=want)
    assert st.pull_iterations == int(pull)
    hops_launches = 0 if kind == "bfs" else 2 + 5 * ((st.iterations + 1 + 3) // 4)
    assert st.advance_launches - hops_launches == (4 if pull else 5)  # 776 entries: the plan always runs
