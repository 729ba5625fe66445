"""grx_neighbor_sample against the oracle of tests/sample_oracle.py: nodes, offsets, src, dst, entries and
the pinned stats with ==, every call made twice, under every lane-group width (GRX_SAMPLE_GROUP 0, 8,
64, 256).  Each case is named for what can go wrong at its shape."""
import ctypes as C
import os

import numpy as np
import pytest

from sample_oracle import EXCLUDE, INCLUDE, csr, mtx_csr, neighbor_sample, sample_plan

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
HUB = 38
INVALID, RUNTIME = -1, -2  # GRX_ERR_INVALID_ARGUMENT, GRX_ERR_RUNTIME
GROUPS = (0, 8, 64, 256)


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


@pytest.fixture(scope="module")
def chesapeake():
    return mtx_csr(CHESAPEAKE)


class forced_group:
    """GRX_SAMPLE_GROUP set around a call and restored behind it."""

    def __init__(self, width):
        self.width = width

    def __enter__(self):
        self.before = os.environ.get("GRX_SAMPLE_GROUP")
        os.environ["GRX_SAMPLE_GROUP"] = str(self.width)

    def __exit__(self, *exc):
        if self.before is None:
            del os.environ["GRX_SAMPLE_GROUP"]
        else:
            os.environ["GRX_SAMPLE_GROUP"] = self.before


def same(got, st, want, fanouts):
    assert got.node_offsets == want["node_offsets"] and got.edge_offsets == want["edge_offsets"]
    for name, mine in (("nodes", got.nodes), ("src", got.src), ("dst", got.dst), ("entries", got.entries)):
        host = mine.cpu().numpy()
        assert str(mine.dtype) == "torch.int32" and host.shape == want[name].shape, name
        bad = np.flatnonzero(host != want[name])
        assert len(bad) == 0, (name, len(bad), bad[:4], host[bad[:4]], want[name][bad[:4]])
    assert st.iterations == want["iterations"] and st.vertices_reached == len(want["nodes"])
    assert st.edges_traversed == len(want["src"]) and st.edges_expanded == want["expanded"]
    assert st.frontier_slots == want["slots"] and len(st.frontier_slots) == len(fanouts)  # levels_recorded


def check(ea, ctx, graph, seeds, fanouts, seed=0, g=None):
    """ea.neighbor_sample under every group width, two calls each that repeat each other, equal to the
    oracle (computed once) -> the oracle's dict."""
    import torch
    ap, aj = graph[0], graph[1]
    if g is None:
        g = ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32))
    want = neighbor_sample(ap, aj, seeds, fanouts, seed)
    for width in GROUPS:
        with forced_group(width):
            first, st = ea.neighbor_sample(ctx, g, seeds, fanouts, seed)
            again, st2 = ea.neighbor_sample(ctx, g, seeds, fanouts, seed)
        same(first, st, want, fanouts)
        for a, b in ((first.nodes, again.nodes), (first.src, again.src), (first.dst, again.dst),
                     (first.entries, again.entries)):
            assert torch.equal(a, b)
        assert (first.node_offsets, first.edge_offsets) == (again.node_offsets, again.edge_offsets)
        assert (st.iterations, st.vertices_reached, st.edges_traversed, st.edges_expanded, st.frontier_slots) == \
            (st2.iterations, st2.vertices_reached, st2.edges_traversed, st2.edges_expanded, st2.frontier_slots)
    return want


# ---- the hand-checked shapes ---------------------------------------------------------------------------

PATH = csr(6, [(v, v + 1) for v in range(5)])
STAR = csr(6, [(0, 1 + k) for k in range(5)])


def test_directed_path_takes_whole_rows_and_stops_at_the_dead_end(ea, ctx):
    want = check(ea, ctx, PATH, [0], [1, 1, 1])
    assert want["nodes"].tolist() == [0, 1, 2, 3] and want["expanded"] == 3
    want = check(ea, ctx, PATH, [4], [1, 1, 1])
    assert want["node_offsets"] == [0, 1, 2, 2, 2] and want["slots"] == [1, 1, 0]
    check(ea, ctx, PATH, [3, 1, 3, 1, 0], [1, 2])  # duplicate seeds


@pytest.mark.parametrize("k", [2, 3])
def test_star_include_and_exclude(ea, ctx, k):
    for seed in (0, 1, 2, 3):
        want = check(ea, ctx, STAR, [0], [k], seed=seed)
        assert len(want["entries"]) == k and want["attempts"] >= 2
    assert sample_plan(5, 2)[0] == INCLUDE and sample_plan(5, 3)[0] == EXCLUDE


# ---- every plan boundary, and the table's worst fill ----------------------------------------------------

FANS = (1, 8, 9, 64, 65, 1024)


@pytest.fixture(scope="module")
def hubs():
    """One hub per (k, d) with d = k, k + 1, 2k - 1, 2k, 2k + 1: hub i's row is leaves 0 .. d - 1, rotated
    by i so that equal positions of different hubs are different vertices."""
    lengths = sorted({d for k in FANS for d in (k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1)})
    n_leaves = max(lengths)
    first = len(lengths)
    e = [(i, first + (j + i) % n_leaves) for i, d in enumerate(lengths) for j in range(d)]
    return csr(first + n_leaves, e), first, lengths


@pytest.mark.parametrize("k", FANS)
def test_rows_at_the_plan_boundaries(ea, ctx, hubs, k):
    graph, first, lengths = hubs
    modes = {sample_plan(d, k)[0] for d in lengths}
    assert modes == {0, INCLUDE, EXCLUDE} or k == 1  # k = 1 has no exclude row
    if k == 1024:
        assert sample_plan(2049, k) == (INCLUDE, 1024) and sample_plan(2047, k) == (EXCLUDE, 1023)  # the largest m
    want = check(ea, ctx, graph, list(range(first)), [k], seed=k)
    assert want["edge_offsets"][1] == sum(min(d, k) for d in lengths)


@pytest.mark.parametrize("k", [32, 33, 40, 256, 257, 300, -1])
def test_rows_on_both_sides_of_the_width_rule(ea, ctx, k):
    """The default rule sends an all-row to 8 lanes up to d = 16 and to a wavefront up to d = 1024, an
    include row by m and an exclude row by d / 2 to 8 lanes up to 32 and to a wavefront up to 256:
    include rows of m = 32, 33, 256, 257, exclude rows of d = 64, 66 (k = 40) and 512, 514 (k = 300),
    and whole rows of 16, 17, 1024, 1025 and 2049 entries (k = -1)."""
    lengths = [16, 17, 64, 66, 512, 514, 1024, 1025, 2049]
    first = len(lengths)
    e = [(i, first + (j * 3 + i) % 2053) for i, d in enumerate(lengths) for j in range(d)]  # 2053 is prime
    want = check(ea, ctx, csr(first + 2053, e), list(range(first)), [k], seed=100 + k)
    assert want["edge_offsets"][1] == sum(d if k < 0 else min(d, k) for d in lengths)


def test_star_of_70000_leaves_is_picked_past_65536(ea, ctx):
    """(r >> 32) * d needs 64 bits at d = 70000."""
    leaves = 70000
    graph = csr(leaves + 1, [(0, 1 + k) for k in range(leaves)])
    past = 0
    for seed in (5, 6, 7):
        want = check(ea, ctx, graph, [0], [16], seed=seed)
        past += int((want["entries"] > 65536).sum())
    assert past > 0


def test_repeated_entries_are_entries_of_their_own_and_loops_name_no_new_vertex(ea, ctx):
    e = [(0, 1), (0, 2), (0, 1), (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2), (2, 2), (2, 1), (2, 3)]
    graph = csr(4, e)
    both = 0
    for seed in range(6):
        want = check(ea, ctx, graph, [0, 2], [2, 2], seed=seed)
        row0 = want["entries"][want["src"] == 0]
        both += int(len(set(row0.tolist()) & {0, 2, 4}) == 2)  # two copies of 0 -> 1 in one sample
    assert both > 0
    check(ea, ctx, graph, [0], [4, -1], seed=1)


def test_isolated_seed_and_empty_list(ea, ctx):
    graph = csr(5, [(0, 1), (1, 0), (3, 3)])
    want = check(ea, ctx, graph, [2, 4], [3, 3])
    assert want["nodes"].tolist() == [2, 4] and want["edge_offsets"] == [0, 0, 0] and want["slots"] == [2, 0]
    want = check(ea, ctx, graph, [3], [1, 1])   # a self loop: an edge, no new vertex
    assert want["nodes"].tolist() == [3] and want["src"].tolist() == [0] and want["dst"].tolist() == [0]
    g = ea.Graph.from_host_csr(*graph)
    got, st = ea.neighbor_sample(ctx, g, [], [3, 3])
    assert got.node_offsets == [0, 0, 0, 0] and got.edge_offsets == [0, 0, 0] and got.nodes.numel() == 0
    assert st.advance_launches == 0 and st.iterations == 0 and st.frontier_slots == []
    empty = ea.Graph.from_host_csr(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    got, st = ea.neighbor_sample(ctx, empty, None, [3])
    assert got.node_offsets == [0, 0, 0] and got.src.numel() == 0 and st.advance_launches == 0


def test_every_vertex_of_chesapeake(ea, ctx, chesapeake):
    want = check(ea, ctx, chesapeake, None, [3])  # NULL list: every vertex expanded, no new vertex
    assert want["node_offsets"] == [0, 39, 39] and want["slots"] == [39]
    want = check(ea, ctx, chesapeake, None, [-1, -1])
    assert want["edge_offsets"] == [0, 340, 340] and want["expanded"] == 340 and want["slots"] == [39, 0]


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_chesapeake_three_hops(ea, ctx, chesapeake, seed):
    want = check(ea, ctx, chesapeake, [HUB, 0, 7], [5, 3, 2], seed=seed)
    assert want["iterations"] == 3 and want["attempts"] > 0


def test_rmat_scale_12_several_workgroups_and_a_sort_of_thousands(ea, ctx):
    g = ea.Graph.rmat(ctx, 12, 16, seed=1)
    ap, aj, _ = g.to_host()
    seeds = np.random.default_rng(3).choice(g.n_rows, 256, replace=False)
    want = check(ea, ctx, (ap, aj), seeds, [10, 5], seed=11, g=g)
    assert want["edge_offsets"][1] > 1024 and want["node_offsets"][3] > want["node_offsets"][2] > want["node_offsets"][1]


def test_a_vertex_sample_does_not_depend_on_the_seed_list(ea, ctx, chesapeake):
    ap, aj, _ = chesapeake
    g = ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32))
    rows = []
    for seeds in ([HUB, 1, 2], [7, HUB], [HUB]):
        got, _ = ea.neighbor_sample(ctx, g, seeds, [8], seed=21)
        at = seeds.index(HUB)
        rows.append(got.entries[got.src == at].cpu().numpy().tolist())
    assert len(rows[0]) == 8 and rows[0] == rows[1] == rows[2]
    other, _ = ea.neighbor_sample(ctx, g, [HUB], [8], seed=22)
    assert other.entries.cpu().numpy().tolist() != rows[0]


# ---- the raw entry point: count-only calls, capacities, errors -----------------------------------------

def test_count_only_call_capacities_and_errors(ea, ctx, chesapeake):
    import torch
    from essentials_amd.api import load_library, _Stats
    lib = load_library()
    ap, aj, _ = chesapeake
    g = ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32))
    seeds = np.asarray([HUB, 0, 7], np.int32)
    fans = np.asarray([5, 3, 2], np.int32)
    want = neighbor_sample(ap, aj, seeds, fans.tolist(), 4)
    n_nodes, n_edges = len(want["nodes"]), len(want["src"])
    node_off, edge_off = np.full(5, -7, np.int64), np.full(4, -7, np.int64)
    nodes = torch.full((n_nodes + 4,), 77, dtype=torch.int32, device="cuda:0")
    src, dst, entry = (torch.full((n_edges + 4,), 77, dtype=torch.int32, device="cuda:0") for _ in range(3))
    torch.cuda.synchronize()

    def raw(ctx_h=ctx._h, g_h=g._h, seeds_p=seeds.ctypes.data, n=3, fans_p=fans.ctypes.data, hops=3,
            nodes_p=nodes.data_ptr(), node_cap=n_nodes, src_p=src.data_ptr(), dst_p=dst.data_ptr(),
            entry_p=entry.data_ptr(), edge_cap=n_edges, node_off_p=node_off.ctypes.data,
            edge_off_p=edge_off.ctypes.data, opt=None, stats=None):
        return lib.grx_neighbor_sample(ctx_h, g_h, seeds_p, n, fans_p, hops, 4, nodes_p, node_cap, src_p, dst_p,
                                       entry_p, edge_cap, node_off_p, edge_off_p, opt, stats)

    # the exact capacities are enough
    assert raw() == 0
    assert node_off.tolist() == want["node_offsets"] and edge_off.tolist() == want["edge_offsets"]
    assert (nodes.cpu().numpy()[:n_nodes] == want["nodes"]).all() and (nodes[n_nodes:] == 77).all()
    assert (dst.cpu().numpy()[:n_edges] == want["dst"]).all() and (dst[n_edges:] == 77).all()
    # count-only: no device output, the same offsets and stats
    node_off[:], edge_off[:] = -7, -7
    st = _Stats()
    assert raw(nodes_p=None, src_p=None, dst_p=None, entry_p=None, node_cap=0, edge_cap=0, stats=C.byref(st)) == 0
    assert node_off.tolist() == want["node_offsets"] and edge_off.tolist() == want["edge_offsets"]
    assert st.vertices_reached == n_nodes and st.edges_traversed == n_edges and st.edges_expanded == want["expanded"]
    assert raw(nodes_p=None, src_p=None, dst_p=None, entry_p=None, node_off_p=None) == 0  # one output is enough
    # one short
    assert raw(edge_cap=n_edges - 1) == RUNTIME
    message = lib.grx_last_error().decode()
    assert "grx_neighbor_sample" in message and "hop 3" in message and str(n_edges) in message
    assert raw(node_cap=n_nodes - 1) == RUNTIME
    message = lib.grx_last_error().decode()
    assert "node_capacity" in message and str(n_nodes) in message
    assert raw(node_cap=2) == RUNTIME and "level 0" in lib.grx_last_error().decode()
    # only the capacities of the arrays that are given count
    assert raw(nodes_p=None, node_cap=0) == 0 and raw(src_p=None, dst_p=None, entry_p=None, edge_cap=0) == 0

    # every host-side error
    nodes.fill_(77)
    src.fill_(77)
    torch.cuda.synchronize()
    assert raw(ctx_h=None) == INVALID and raw(g_h=None) == INVALID and raw(fans_p=None) == INVALID
    assert raw(n=-1) == INVALID and raw(seeds_p=None) == INVALID
    assert raw(seeds_p=np.asarray([1, 39, 3], np.int32).ctypes.data) == INVALID
    assert raw(seeds_p=np.asarray([1, -1, 3], np.int32).ctypes.data) == INVALID
    assert raw(hops=0) == INVALID and raw(hops=-1) == INVALID
    many = np.full(65, 2, np.int32)
    assert raw(fans_p=many.ctypes.data, hops=65) == INVALID
    for bad in (0, -2, 1025):
        assert raw(fans_p=np.asarray([5, bad, 2], np.int32).ctypes.data) == INVALID
    wide = ea.Graph.from_host_csr(ap, aj, np.ones(len(aj), np.float32), n_cols=40)
    assert raw(g_h=wide._h) == INVALID
    assert raw(node_cap=-1) == INVALID and raw(edge_cap=-1) == INVALID
    assert raw(nodes_p=None, src_p=None, dst_p=None, entry_p=None, node_off_p=None, edge_off_p=None) == INVALID
    assert b"grx_neighbor_sample" in lib.grx_last_error()
    assert (nodes == 77).all() and (src == 77).all()  # nothing was written
    with pytest.raises(ea.EngineError):
        ea.neighbor_sample(ctx, g, [1], [2], options=ea.Options(max_iterations=3))
    with pytest.raises(ea.EngineError):
        ea.neighbor_sample(ctx, g, [1], [0])
    # an empty list zeroes the offsets and the stats and leaves the device outputs alone
    st = _Stats()
    st.iterations = 5
    node_off[:], edge_off[:] = -7, -7
    assert raw(n=0, stats=C.byref(st)) == 0
    assert st.iterations == 0 and node_off.tolist() == [0] * 5 and edge_off.tolist() == [0] * 4
    assert (nodes == 77).all()
    # the 64 hops the stats can record
    got, st = ea.neighbor_sample(ctx, g, [HUB], [1] * 64, seed=3)
    assert len(st.frontier_slots) == 64 and got.edge_offsets[-1] == st.edges_traversed
