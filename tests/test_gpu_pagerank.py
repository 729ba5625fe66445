"""grx_pagerank per vertex: every device form of the PageRank client against the float64 restatement
of tests/pr_oracle.py after exactly T iterations (tol = 0 is never met: `err < tol` is false), within
the rounding bound derived there -- |got - p| <= allowed at EVERY vertex, whatever order the float adds
took.  tests/test_pr_oracle.py proves on the CPU that a correct float32 run uses at most half of that
bound and that a lost or doubled edge, a confused transpose, lost dangling mass, ranks handed over in
the wrong numbering, an iteration more or less and a stale read each exceed four times it on these
graphs.  A ratio above 1 here is a defect of the device code, not of the bound.

Forms: push under every load balance; push and pull walking the destination-sorted list (forced onto
these small graphs; GRX_HOT_FIRST=1 puts both on the hot-first copy as well, which the size rule
alone would not at these sizes, so pr_problem_t::deliver() is under test); pull over the
per-destination lists (row_group_sum_kernel, hub_chunk_sum_kernel); both with the list switched off;
the partitioned scatter at world 1 under both host loops."""
import numpy as np
import pytest

import pr_oracle as po

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ALPHA = 0.85
TS = (1, 3, 10)
ALL_LB = ["block_mapped", "merge_path", "bucketing", "work_stealing", "thread_mapped", "warp_mapped"]
BY_TOLERANCE = ("rmat10", "dangling")      # the graphs of the runs that stop by tol = 1e-6


@pytest.fixture(scope="module")
def ea():
    import essentials_amd
    return essentials_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.fixture(scope="module")
def ctx(ea, torch):
    return ea.Context(0)


class Wanted:
    """The graphs and, computed once and never changed, their references."""

    def __init__(self, oracle):
        self.graphs = dict(po.cases())
        _, Ap, Aj, Ax = oracle.rmat_csr(10, 8, 3, 5, False)
        self.graphs["rmat10"] = (np.ascontiguousarray(Ap), np.ascontiguousarray(Aj), np.ascontiguousarray(Ax))
        self.indeg = {k: po.in_degrees(g[0], g[1]) for k, g in self.graphs.items()}
        self._ref, self._stop = {}, {}

    def reference(self, name, T):
        if (name, T) not in self._ref:
            p, allowed = po.reference(*self.graphs[name], ALPHA, T)
            p.setflags(write=False)
            allowed.setflags(write=False)
            self._ref[name, T] = (p, allowed)
        return self._ref[name, T]

    def stop(self, name, tol):
        if (name, tol) not in self._stop:
            self._stop[name, tol] = po.iterations_to_tolerance(*self.graphs[name], ALPHA, tol)
        return self._stop[name, tol]

    def check(self, got, name, T, what):
        """Largest |got - p| / allowed; fails naming the worst vertex."""
        p, allowed = self.reference(name, T)
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == p.shape
        r = po.ratio(got, p, allowed)
        v = int(np.argmax(r))
        assert (np.abs(got.astype(np.float64) - p) <= allowed).all(), (
            f"{what} {name} T={T}: vertex {v} (in-degree {int(self.indeg[name][v])}) is off by "
            f"{r[v]:.3f} x allowed; {int((r > 1).sum())} vertices beyond the bound")
        return float(r[v])


@pytest.fixture(scope="module")
def wanted(oracle):
    return Wanted(oracle)


def host(t):
    return t.cpu().numpy()


def sweep(ea, c, wanted, what, pull=False, repeats=1, then_pull=False, **options):
    """Every graph, T in TS (`repeats` runs each on the same context and graph: the second one walks
    what the first one left), then one run by tolerance; -> the largest ratio.  then_pull: the
    transpose is attached to the graph the push runs used, and the pull form runs on it as well."""
    top = 0.0
    for name, (ap, aj, aw) in wanted.graphs.items():
        G = ea.Graph.from_host_csr(ap, aj, aw)
        if pull:
            G.build_in_edges(c)                        # every graph here is directed
        for T in TS:
            for again in range(repeats):
                got, st = ea.pagerank(c, G, ALPHA, 0.0, options=ea.Options(
                    max_iterations=T, direction_optimized=pull, **options))
                assert st.iterations == T, (what, name, T, st.iterations)
                assert st.pull_iterations == (T if pull else 0)
                top = max(top, wanted.check(host(got), name, T, f"{what} run {again}"))
        if name in BY_TOLERANCE:
            got, st = ea.pagerank(c, G, ALPHA, 1e-6, options=ea.Options(direction_optimized=pull, **options))
            assert abs(st.iterations - wanted.stop(name, 1e-6)) <= 1, (what, name, st.iterations)
            top = max(top, wanted.check(host(got), name, st.iterations, f"{what} by tolerance"))
        if then_pull:
            G.build_in_edges(c)
            for T in TS:
                got, st = ea.pagerank(c, G, ALPHA, 0.0, options=ea.Options(max_iterations=T,
                                                                           direction_optimized=True))
                assert st.iterations == st.pull_iterations == T, (what, name, T, st.iterations)
                top = max(top, wanted.check(host(got), name, T, f"{what}, then pull"))
        G.close()
    print(f"\n[pagerank] {what}: largest |got - p| / allowed = {top:.3f}")
    return top


@pytest.mark.parametrize("lb", ALL_LB)
def test_push(ea, ctx, wanted, lb):
    """The push scatter row by row (these graphs are far below the size at which the list switches
    on by itself): one float atomic per edge, out_scale_kernel, the dangling-mass reduction."""
    sweep(ea, ctx, wanted, f"push {lb}", load_balance=ea.LoadBalance[lb])


FORCED = {"list": {}, "list, caller's numbering": {"GRX_PR_HOT_FIRST": "0"},
          "list, plain loads": {"GRX_BY_DESTINATION_STREAM": "0"}}


@pytest.mark.parametrize("lb", ["block_mapped", "merge_path"])
@pytest.mark.parametrize("variant", list(FORCED))
def test_push_and_pull_over_the_destination_sorted_list(ea, torch, wanted, monkeypatch, variant, lb):
    """expand_kernel over the sorted list with the adds of neighbouring lanes combined, on the
    hot-first copy (ranks gathered back by deliver()); each graph twice on the same context, the
    second run on the remembered list.  Then in the caller's own numbering, and with plain loads in
    place of the streaming ones."""
    monkeypatch.setenv("GRX_BY_DESTINATION", "1")
    monkeypatch.setenv("GRX_HOT_FIRST", "1")           # the size rule alone says no below 2^16 vertices
    for key, value in FORCED[variant].items():
        monkeypatch.setenv(key, value)
    c = ea.Context(0)                                  # reads GRX_BY_DESTINATION
    sweep(ea, c, wanted, f"push {lb} over the {variant}", repeats=2, then_pull=lb != "block_mapped",
          load_balance=ea.LoadBalance[lb])
    if lb == "block_mapped":                           # the pull form has no load balance
        sweep(ea, c, wanted, f"pull over the {variant}", pull=True, repeats=2)
    c.close()


def test_pull_over_the_per_destination_lists(ea, ctx, wanted, monkeypatch):
    """row_group_sum_kernel (16 lanes per in-row below RED_HUB = 256 entries) and
    hub_chunk_sum_kernel (chunks of RED_CHUNK = 2048): hub(m) puts in-rows of 255 .. 4100 entries
    around both, short_rows() around the 16-lane stripes."""
    monkeypatch.setenv("GRX_PR_PULL_WALK", "0")
    sweep(ea, ctx, wanted, "pull over the per-destination lists", pull=True)


def test_push_and_pull_with_the_list_switched_off(ea, torch, wanted, monkeypatch):
    """GRX_BY_DESTINATION=0: the push scatter row by row; the pull form, which then has no list to
    walk, sums over the attached in-rows."""
    monkeypatch.setenv("GRX_BY_DESTINATION", "0")
    c = ea.Context(0)
    sweep(ea, c, wanted, "push, list off", repeats=2)
    sweep(ea, c, wanted, "pull, list off", pull=True, repeats=2)
    c.close()


def _partitioned(wanted, what, make, torch):
    top = 0.0
    for name, (ap, aj, aw) in wanted.graphs.items():
        n = len(ap) - 1
        run, done = make(ap, aj, aw, n)
        p = torch.empty(n, dtype=torch.float32, device="cuda")
        for T in TS:
            st = run(p, ALPHA, 0.0, T)
            assert st["iterations"] == T, (what, name, T, st)
            top = max(top, wanted.check(host(p), name, T, what))
        if name in BY_TOLERANCE:
            st = run(p, ALPHA, 1e-6, 0)
            assert abs(st["iterations"] - wanted.stop(name, 1e-6)) <= 1, (what, name, st)
            top = max(top, wanted.check(host(p), name, st["iterations"], f"{what} by tolerance"))
        done()
    print(f"\n[pagerank] {what}: largest |got - p| / allowed = {top:.3f}")


def test_partitioned_scatter_world1_host_loop(ea, ctx, torch, wanted):
    """grx_pagerank_partitioned_scatter under the Python loop (PartitionedPageRank), one rank owning
    every row."""
    from essentials_amd.distributed import HipKernels, PartitionedPageRank

    def make(ap, aj, aw, n):
        g = ea.Graph.from_host_csr(ap, aj, aw)
        loop = PartitionedPageRank(HipKernels(ctx, g), None, 0, 1, n, 0, n, "cuda:0")
        return (lambda p, alpha, tol, T: loop.run(p, alpha, tol, max_iterations=T)), g.close

    _partitioned(wanted, "partitioned scatter, python loop", make, torch)


def test_partitioned_scatter_world1_cpp_loop(ea, torch, wanted):
    """The same scatter under the C++ loop (PartitionedPlan.pagerank: all-reduce and
    pagerank_update_kernel on the engine's stream) in a job of one."""
    c = ea.Context(0)
    c.attach_rccl(0, 1, ea.Context.unique_id())

    def make(ap, aj, aw, n):
        g = ea.Graph.from_host_csr(ap, aj, aw)
        plan = ea.PartitionedPlan(c, g, 0, n)

        def done():
            plan.close()
            g.close()
        return (lambda p, alpha, tol, T: plan.pagerank(p, alpha, tol, max_iterations=T)), done

    _partitioned(wanted, "partitioned scatter, c++ loop", make, torch)
    c.detach()
    c.close()


def test_smallest_graphs_rank_one_over_n(ea, ctx, monkeypatch):
    """n = 1 (a self loop) and graphs of 1, 2, 3 and 5 vertices without edges: every rank is 1/n after
    any number of iterations, in the reference exactly and on the device within `allowed` (a few
    2**-24 of 1/n), by the push scatter and by the sums over the (empty) in-rows."""
    monkeypatch.setenv("GRX_PR_PULL_WALK", "0")
    graphs = {"self loop": po.tiny(1)}
    graphs.update({f"{n} vertices, no edges": po.edgeless(n) for n in (1, 2, 3, 5)})
    for name, (ap, aj, aw) in graphs.items():
        n = len(ap) - 1
        G = ea.Graph.from_host_csr(ap, aj, aw)
        G.build_in_edges(ctx)
        for T in TS:
            p, allowed = po.reference(ap, aj, aw, ALPHA, T)
            # an iteration adds at most (n_dangling + log2 n + 4) + 4 + 5 + 3 <= n + 16 units of u
            assert np.abs(p - 1.0 / n).max() < 1e-15 and allowed.max() <= 2 * (n + 16) * T * po.U / n
            for pull in (False, True):
                got, st = ea.pagerank(ctx, G, ALPHA, 0.0, options=ea.Options(max_iterations=T,
                                                                             direction_optimized=pull))
                assert st.iterations == T
                assert (np.abs(host(got).astype(np.float64) - 1.0 / n) <= allowed).all(), (name, T, pull, host(got))
        G.close()
