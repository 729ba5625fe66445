"""grx_random_walk against the oracle of tests/walk_oracle.py: walks and stats with ==, every call made
twice.  Each case is named for what can go wrong at its shape."""
import ctypes as C
import os

import numpy as np
import pytest

from walk_oracle import csr, mtx_csr, random_walk

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
HUB = 38
INVALID = -1  # GRX_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def ctx(ea):
    return ea.Context(0)


@pytest.fixture(scope="module")
def chesapeake():
    ap, aj, _ = mtx_csr(CHESAPEAKE)
    return ap, aj, (1 + (np.arange(len(aj)) * 7) % 5).astype(np.float32)


def check(ea, ctx, csr3, starts, length, cap=None, **kw):
    """Two calls of ea.random_walk that repeat each other, and equal the oracle: walks and stats.
    -> (walks as numpy, Stats, the oracle's dict)."""
    import torch
    ap, aj, ax = csr3
    g = ea.Graph.from_host_csr(ap, aj, ax)
    want = random_walk(ap, aj, ax, starts, length, **kw, **({} if cap is None else {"cap": cap}))
    first = None
    for _ in range(2):
        w, st = ea.random_walk(ctx, g, starts, length, **kw)
        assert str(w.dtype) == "torch.int32" and tuple(w.shape) == want["walks"].shape
        host = w.cpu().numpy()
        bad = np.flatnonzero((host != want["walks"]).any(1))
        assert len(bad) == 0, (len(bad), bad[:4], host[bad[:2]], want["walks"][bad[:2]])
        assert st.iterations == want["iterations"] and st.vertices_reached == want["full"]
        assert st.edges_traversed == want["steps"] == int((host >= 0).sum()) - len(host)
        assert st.edges_expanded == want["attempts"]
        assert st.frontier_slots == want["slots"]  # its length is levels_recorded
        assert st.advance_launches == want["launches"]
        if first is None:
            first = (w.clone(), st)
        else:
            assert torch.equal(w, first[0])
    return host, first[1], want


# ---- dead ends and padding -----------------------------------------------------------------------------

PATH = csr(6, [(v, v + 1) for v in range(5)])


@pytest.mark.parametrize("kw", [{}, {"weighted": True}, {"p": 0.25, "q": 4.0}, {"weighted": True, "p": 4.0, "q": 0.25}])
def test_directed_path_pads_behind_the_dead_end(ea, ctx, kw):
    host, st, _ = check(ea, ctx, PATH, [0, 3, 5], 4, seed=9, **kw)
    assert host.tolist() == [[0, 1, 2, 3, 4], [3, 4, 5, -1, -1], [5, -1, -1, -1, -1]]
    assert st.iterations == 4 and st.frontier_slots == [2, 2, 1, 1]


def test_length_zero_writes_the_starts_only(ea, ctx):
    host, st, _ = check(ea, ctx, PATH, [4, 0, 4], 0, weighted=True, p=2.0)
    assert host.tolist() == [[4], [0], [4]] and st.iterations == 0 and st.frontier_slots == []
    assert st.vertices_reached == 3 and st.advance_launches == 1


def test_isolated_start_and_every_vertex(ea, ctx):
    ap, aj, ax = csr(5, [(0, 1), (1, 0), (3, 3)])
    host, _, _ = check(ea, ctx, (ap, aj, ax), [2, 4, 0], 3)
    assert host[:2].tolist() == [[2, -1, -1, -1], [4, -1, -1, -1]] and host[2].tolist() == [0, 1, 0, 1]
    host, _, _ = check(ea, ctx, (ap, aj, ax), None, 3, p=0.5, q=2.0)  # NULL list: every vertex
    assert host[:, 0].tolist() == [0, 1, 2, 3, 4] and host[3].tolist() == [3, 3, 3, 3]  # a self loop stays put


# ---- 64-bit index arithmetic ---------------------------------------------------------------------------

def test_star_of_70000_leaves_is_picked_past_65536(ea, ctx):
    """(r >> 32) * d needs 64 bits at d = 70000; the second step returns to the hub."""
    leaves = 70000
    e = [(0, 1 + k) for k in range(leaves)] + [(1 + k, 0) for k in range(leaves)]
    host, st, _ = check(ea, ctx, csr(leaves + 1, e), [0] * 2048, 2, seed=5)
    assert (host[:, 1] > 65536).sum() > 50 and (host[:, 2] == 0).all() and host[:, 1].min() >= 1
    assert st.vertices_reached == 2048


# ---- multigraph and self loops -------------------------------------------------------------------------

def test_repeated_entries_count_each_time_and_loops_are_steps(ea, ctx):
    e = [(0, 1), (0, 2), (0, 1), (0, 0), (1, 0), (2, 0), (2, 2)]
    g3 = csr(3, e)
    host, _, want = check(ea, ctx, g3, [0] * 4096, 1, seed=2)
    counts = np.bincount(host[:, 1], minlength=3)
    assert abs(counts[1] / counts[2] - 2) < 0.25 and abs(counts[0] / counts[2] - 1) < 0.2  # per the oracle
    for kw in ({}, {"p": 0.125, "q": 8.0}, {"weighted": True, "p": 8.0, "q": 0.125}):
        check(ea, ctx, g3, [0, 1, 2] * 50, 9, seed=3, **kw)


# ---- chesapeake ----------------------------------------------------------------------------------------

def test_loader_keeps_the_row_order_the_oracle_assumes(ea, chesapeake):
    ap, aj, _ = chesapeake
    gp, gj, _ = ea.Graph.from_mtx(CHESAPEAKE).to_host()
    assert (gp == ap).all() and (gj == aj).all()


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_chesapeake_uniform(ea, ctx, chesapeake, seed):
    host, st, _ = check(ea, ctx, chesapeake, None, 16, seed=seed)
    assert st.iterations == 16 and st.vertices_reached == 39 and st.edges_expanded == 39 * 16


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25)])
def test_chesapeake_node2vec(ea, ctx, chesapeake, p, q, weighted):
    _, st, _ = check(ea, ctx, chesapeake, None, 16, seed=6, weighted=weighted, p=p, q=q)
    assert st.edges_expanded > st.edges_traversed == 39 * 16


@pytest.mark.parametrize("weighted", [False, True])
def test_membership_does_not_depend_on_row_order(ea, ctx, chesapeake, weighted):
    """Every row shuffled: the walks are those of the oracle on the shuffled CSR."""
    ap, aj, ax = chesapeake
    rng = np.random.default_rng(8)
    sj, sx = aj.copy(), ax.copy()
    for v in range(len(ap) - 1):
        order = ap[v] + rng.permutation(ap[v + 1] - ap[v])
        sj[ap[v]:ap[v + 1]], sx[ap[v]:ap[v + 1]] = aj[order], ax[order]
    check(ea, ctx, (ap, sj, sx), None, 16, seed=6, weighted=weighted, p=0.25, q=4.0)


def test_membership_looks_in_the_row_of_prev(ea, ctx):
    """0 -> {1, 2, 3}, 1 -> {2, 3, 4}, the others -> 0.  At 1, from 0: 2 and 3 are entries of row 0
    (adj) although neither has an entry to 0's row the other way round; 4 is far."""
    e = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (1, 4), (2, 0), (3, 0), (4, 0)]
    host, _, _ = check(ea, ctx, csr(5, e), [0] * 3000, 2, seed=1, p=8.0, q=8.0)
    second = host[host[:, 1] == 1, 2]
    counts = np.bincount(second, minlength=5)
    # adj = 1, far = 1/8: looking prev up in row x instead would make 4 (4 -> 0 exists) as likely as 2 and 3
    assert counts[2] > 4 * counts[4] and counts[3] > 4 * counts[4] and counts[4] > 0


# ---- weighted ------------------------------------------------------------------------------------------

def test_weighted_rows_with_block_boundaries_and_zeros(ea, ctx):
    """Row 0: 130 entries of weight k % 7 (blocks end at 64 and 128); row 1: 4097 entries of weight
    1 + k % 64 (65 blocks, the last of one entry); row 2: all zeros, a dead end."""
    e = [(0, 3 + k) for k in range(130)] + [(1, 3 + k) for k in range(4097)] + [(2, 3 + k) for k in range(70)]
    w = [k % 7 for k in range(130)] + [1 + k % 64 for k in range(4097)] + [0] * 70
    n = 3 + 4097
    e += [(3 + k, k % 3) for k in range(4097)]
    w += [1] * 4097
    host, st, _ = check(ea, ctx, csr(n, e, w), [0] * 1500 + [1] * 1500 + [2] * 8, 3, seed=4, weighted=True)
    first = host[:1500, 1] - 3
    assert (first % 7 != 0).all() and first.max() > 128 and ((first >= 64) & (first < 128)).any()
    assert (host[1500:3000, 1] - 3 > 4032).any()
    assert (host[3000:, 1:] == -1).all() and st.frontier_slots[0] == 3000


def test_weighted_rmat(ea, ctx):
    g = ea.Graph.rmat(ctx, 10, 16, seed=1, weight_seed=7)
    ap, aj, ax = g.to_host()
    starts = np.arange(4096) % g.n_rows
    want = random_walk(ap, aj, ax, starts, 8, seed=11, weighted=True)
    for _ in range(2):
        w, st = ea.random_walk(ctx, g, starts, 8, seed=11, weighted=True)
        assert (w.cpu().numpy() == want["walks"]).all()
        assert (st.iterations, st.vertices_reached, st.edges_traversed, st.edges_expanded, st.frontier_slots) == \
            (want["iterations"], want["full"], want["steps"], want["attempts"], want["slots"])


# ---- the attempt cap -----------------------------------------------------------------------------------

def test_attempt_cap(ea, ctx, chesapeake, monkeypatch):
    args = dict(starts=[HUB] * 64, length=6, seed=3, p=8.0, q=0.125)
    default, _, _ = check(ea, ctx, chesapeake, **args)
    monkeypatch.setenv("GRX_WALK_MAX_ATTEMPTS", "2")
    capped, st, _ = check(ea, ctx, chesapeake, cap=2, **args)
    differ = int((capped != default).any(1).sum())
    print(f"{differ} of 64 rows differ")
    assert differ > 0 and st.edges_expanded <= 64 + 2 * 64 * 5


# ---- independence --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{}, {"weighted": True, "p": 0.5, "q": 2.0}])
def test_a_walk_does_not_depend_on_the_rest_of_the_list(ea, ctx, chesapeake, kw):
    ap, aj, ax = chesapeake
    g = ea.Graph.from_host_csr(ap, aj, ax)
    starts = (np.arange(1000) * 5) % 39
    whole, _ = ea.random_walk(ctx, g, starts, 10, seed=12, **kw)
    for k in (1, 300, 513):  # within one workgroup of 256 walks and across several
        part, _ = ea.random_walk(ctx, g, starts[:k], 10, seed=12, **kw)
        assert (part == whole[:k]).all()
    repeated, _ = ea.random_walk(ctx, g, [3, 7], 10, seed=12, walks_per_start=3, **kw)
    listed, _ = ea.random_walk(ctx, g, [3, 3, 3, 7, 7, 7], 10, seed=12, **kw)
    assert (repeated == listed).all() and (repeated[0] != repeated[1]).any()


# ---- errors --------------------------------------------------------------------------------------------

def test_errors_are_found_before_anything_runs(ea, ctx, chesapeake):
    import torch
    from essentials_amd.api import load_library, _Stats
    lib = load_library()
    ap, aj, ax = chesapeake
    g = ea.Graph.from_host_csr(ap, aj, ax)
    out = torch.full((4, 3), 77, dtype=torch.int32, device="cuda:0")
    one = np.asarray([1, 2, 3, 4], np.int32)

    def raw(ctx_h=ctx._h, g_h=g._h, starts=one.ctypes.data, n=4, length=2, weighted=0, p=1.0, q=1.0,
            walks=out.data_ptr()):
        return lib.grx_random_walk(ctx_h, g_h, starts, n, length, 0, weighted, p, q, walks, None, None)

    assert raw() == 0 and (out.cpu().numpy()[:, 0] == one).all()
    out.fill_(77)
    torch.cuda.synchronize()
    assert raw(ctx_h=None) == INVALID and raw(g_h=None) == INVALID
    assert raw(n=-1) == INVALID and raw(starts=None) == INVALID and raw(length=-1) == INVALID
    assert raw(starts=np.asarray([1, 2, 39, 4], np.int32).ctypes.data) == INVALID
    assert raw(starts=np.asarray([1, -1, 3, 4], np.int32).ctypes.data) == INVALID
    for bad in (float("nan"), 0.1, 8.5, -1.0, 0.0, float("inf")):
        assert raw(p=bad) == INVALID and raw(q=bad) == INVALID
    assert raw(walks=None) == INVALID
    assert b"grx_random_walk" in lib.grx_last_error()
    assert (out == 77).all()  # nothing was written
    wide = ea.Graph.from_host_csr(ap, aj, ax, n_cols=40)
    assert raw(g_h=wide._h) == INVALID
    with pytest.raises(ea.EngineError):
        ea.random_walk(ctx, g, [1], 2, options=ea.Options(max_iterations=3))
    with pytest.raises(ea.EngineError):
        ea.random_walk(ctx, g, [1], 2, p=9.0)
    # an empty list and an empty graph are fine, and zero the stats
    st = _Stats()
    st.iterations = 5
    assert lib.grx_random_walk(ctx._h, g._h, one.ctypes.data, 0, 2, 0, 0, 1.0, 1.0, None, None, C.byref(st)) == 0
    assert st.iterations == 0
    w, st = ea.random_walk(ctx, g, [], 4)
    assert tuple(w.shape) == (0, 5) and st.advance_launches == 0
    empty = ea.Graph.from_host_csr(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    w, st = ea.random_walk(ctx, empty, None, 4)
    assert tuple(w.shape) == (0, 5) and st.advance_launches == 0


def test_a_wrong_walks_tensor_is_refused(ea, ctx, chesapeake):
    import torch
    g = ea.Graph.from_host_csr(*chesapeake)
    with pytest.raises(TypeError):
        ea.random_walk(ctx, g, [1, 2], 3, walks=torch.empty((2, 4), dtype=torch.int64, device="cuda:0"))
    with pytest.raises(TypeError):
        ea.random_walk(ctx, g, [1, 2], 3, walks=np.empty((2, 4), np.int32))
    with pytest.raises(ValueError):
        ea.random_walk(ctx, g, [1, 2], 3, walks=torch.empty((2, 5), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        ea.random_walk(ctx, g, [1, 2], 3, walks=torch.empty((2, 8), dtype=torch.int32, device="cuda:0")[:, ::2])
    with pytest.raises(ValueError):
        ea.random_walk(ctx, g, [1, 2], 3, walks=torch.empty((2, 4), dtype=torch.int32))
    mine = torch.empty(8, dtype=torch.int32, device="cuda:0")
    w, _ = ea.random_walk(ctx, g, [1, 2], 3, walks=mine)
    assert w.data_ptr() == mine.data_ptr() and tuple(w.shape) == (2, 4) and w[:, 0].tolist() == [1, 2]
