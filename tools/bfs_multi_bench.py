#!/usr/bin/env python3
"""grx_bfs_multi against 64 calls of grx_bfs on symmetrised RMAT-16 / 20 / 22 as generated (edge
factor 16, seed 1), the same 64 sources (random, distinct, seeded) for both legs, one process.

Leg one: bfs_multi in four forms -- summaries only and with depths, push only and
direction-optimised (default do_alpha) -- each the best of 3 whole calls after a warm one, with the
kernels alone (collect_kernel_time), the levels, the pulled levels, and edges_traversed over the sum
of the 64 single searches' edges_traversed: the share of the edge stream the batch still walks.
Leg two: 64 grx_bfs calls on the same handle with default options, the best of 3 sums after a warm
pass.  Every form's depths are compared with the single searches' before a time is printed.  Below
each graph's rows: the active vertices per level of the batch, beside the mean frontier per level of
the single searches.  Nothing here is a pass condition.

    python tools/bfs_multi_bench.py [--out FILE] [scale ...]    (default: 16 20 22, profiles/bfs_multi_bench.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "bfs_multi_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scales = [int(x) for x in args] or [16, 20, 22]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    emit(f"{'graph':>7s} {'V':>8s} {'nnz':>10s} {'form':>22s} {'best_ms':>8s} {'kernel_ms':>9s} {'levels':>6s} {'pulls':>5s} "
         f"{'launch':>6s} {'traversed':>11s} {'expanded':>11s} {'trav/single':>11s} {'single64_ms':>11s} {'single/multi':>12s}")
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 0)
        sources = np.random.default_rng(64).choice(g.n_rows, 64, replace=False).astype(np.int32)
        # leg two: 64 single searches
        singles = torch.empty((64, g.n_rows), dtype=torch.int32, device="cuda")
        best_single, single_traversed, single_slots = None, 0, np.zeros(64)
        for attempt in range(4):  # the first pass warms (and builds what grx_bfs keeps on the handle)
            total, single_traversed, single_slots = 0.0, 0, np.zeros(64)
            for i, s in enumerate(sources):
                _, st = ea.bfs(ctx, g, int(s), distances=singles[i])
                total += st.elapsed_ms
                single_traversed += st.edges_traversed
                single_slots[:len(st.frontier_slots)] += st.frontier_slots
            if attempt and (best_single is None or total < best_single):
                best_single = total
        # leg one
        depths = torch.empty((64, g.n_rows), dtype=torch.int32, device="cuda")
        slots = []
        for want_depths in (False, True):
            for optimized in (False, True):
                opt = ea.Options(collect_kernel_time=True, direction_optimized=optimized)
                best = None
                for attempt in range(4):
                    got, summary, st = ea.bfs_multi(ctx, g, sources, depths=depths if want_depths else None,
                                                    want_depths=want_depths, options=opt)
                    if attempt and (best is None or st.elapsed_ms < best.elapsed_ms):
                        best = st
                if want_depths:
                    assert torch.equal(got, singles)
                reached = (singles != ea.INT_UNREACHED).sum(1).cpu().numpy()
                assert (summary["reached"] == reached).all()
                slots = best.frontier_slots
                form = ("depths" if want_depths else "summaries") + (", optimised" if optimized else ", push")
                emit(f"{'rmat%d' % scale:>7s} {g.n_rows:8d} {g.nnz:10d} {form:>22s} {best.elapsed_ms:8.3f} "
                     f"{best.advance_kernel_ms:9.3f} {best.iterations:6d} {best.pull_iterations:5d} "
                     f"{best.advance_launches:6d} {best.edges_traversed:11d} {best.edges_expanded:11d} "
                     f"{best.edges_traversed / max(single_traversed, 1):11.4f} {best_single:11.3f} "
                     f"{best_single / best.elapsed_ms:12.2f}")
        emit(f"  rmat{scale} levels, active vertices of the batch: {slots}")
        emit(f"  rmat{scale} levels, mean frontier of a single search: {[round(float(x) / 64, 1) for x in single_slots[:len(slots)]]}")
        del g, singles, depths
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
