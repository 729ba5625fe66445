#!/usr/bin/env python3
"""grx_truss on the simple graph of symmetric RMAT-16 / 18 / 20 (edge factor 16, seeds 1 / 7): the
edges m, the largest trussness, levels, kernel launches, row entries read per CSR entry, the best of
3 whole calls, its kernels (collect_kernel_time) and its three phases (the copy with the edge ids,
the support pass, the peel with the scatter), the best of 3 without the event pairs, and grx_tc and
grx_kcore on the same handle as yardsticks.  No time is a pass condition.

    python tools/truss_bench.py [scale ...]      (default: 16 18 20)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import essentials_amd as ea


def measure(ctx, g):
    values = torch.empty(g.nnz, dtype=torch.int32, device="cuda")
    opts = ea.Options(collect_kernel_time=True)
    _, largest, first = ea.truss(ctx, g, values, options=opts)
    best = None
    for _ in range(3):
        _, again, st = ea.truss(ctx, g, values, options=opts)
        assert again == largest and st.edges_expanded == first.edges_expanded
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    plain = min(ea.truss(ctx, g, values)[2].elapsed_ms for _ in range(3))  # without the event pairs
    return largest, first, best, plain


def main():
    scales = [int(x) for x in sys.argv[1:]] or [16, 18, 20]
    ctx = ea.Context(0)
    print(f"{'graph':>14s} {'V':>8s} {'nnz':>9s} {'m':>9s} {'truss':>5s} {'levels':>6s} {'launch':>6s} {'read/nnz':>8s} "
          f"{'first_ms':>9s} {'best_ms':>8s} {'kernel_ms':>9s} {'copy_ms':>8s} {'supp_ms':>8s} {'peel_ms':>8s} "
          f"{'plain_ms':>8s} {'tc_ms':>7s} {'kcore_ms':>8s} {'truss/tc':>8s}", flush=True)
    for s in scales:
        g = ea.Graph.rmat(ctx, s, 16, 1, 7).simple(ctx)
        largest, first, best, plain = measure(ctx, g)
        tc_ms = min(ea.tc(ctx, g)[2].elapsed_ms for _ in range(3))
        kcore_ms = min(ea.kcore(ctx, g)[2].elapsed_ms for _ in range(3))
        copy_us, support_us, peel_us = best.frontier_slots
        print(f"{'rmat%d.simple' % s:>14s} {g.n_rows:8d} {g.nnz:9d} {best.edges_traversed:9d} {largest:5d} "
              f"{best.iterations:6d} {best.advance_launches:6d} {best.edges_expanded / g.nnz:8.2f} "
              f"{first.elapsed_ms:9.3f} {best.elapsed_ms:8.3f} {best.advance_kernel_ms:9.3f} {copy_us / 1e3:8.3f} "
              f"{support_us / 1e3:8.3f} {peel_us / 1e3:8.3f} {plain:8.3f} {tc_ms:7.3f} {kcore_ms:8.3f} "
              f"{plain / tc_ms:8.1f}", flush=True)
        del g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
