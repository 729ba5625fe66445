#!/usr/bin/env python3
"""grx_cc on chesapeake, symmetric RMAT-20 / 22 / 24 as generated and directed RMAT-22 (edge factor
16, seeds 1 / 7): components, size of the largest, kernel launches, the first call, the best of 3
whole calls with and without the event pairs of collect_kernel_time (and the slowest of those 3:
the spread), the kernels alone, edges_expanded / nnz; the same with GRX_CC_SAMPLE_ROUNDS=0 (hook
every entry, leave no row out); and grx_bfs from the vertex of largest degree on the same handle in
the same process, best of 3 after a warm call -- the yardstick this algorithm is held against.

    python tools/cc_bench.py [scale ...]      (default: 20 22 24)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(ctx, g, labels):
    timed = ea.Options(collect_kernel_time=True)
    _, count, first = ea.cc(ctx, g, labels, options=timed)
    best = None
    for _ in range(3):
        _, again, st = ea.cc(ctx, g, labels, options=timed)
        assert again == count
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    plain = sorted(ea.cc(ctx, g, labels)[2].elapsed_ms for _ in range(3))  # without the event pairs
    return count, first, best, plain


def main():
    scales = [int(x) for x in sys.argv[1:]] or [20, 22, 24]
    ctx = ea.Context(0)
    graphs = [("chesapeake", lambda: ea.Graph.from_mtx(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")))]
    graphs += [(f"rmat{s}", lambda s=s: ea.Graph.rmat(ctx, s, 16, 1, 7)) for s in scales]
    graphs += [("rmat22.directed", lambda: ea.Graph.rmat(ctx, 22, 16, 1, 7, symmetrize=False))]
    print(f"{'graph':>16s} {'rounds':>6s} {'V':>9s} {'nnz':>11s} {'components':>10s} {'largest':>9s} {'launch':>6s} "
          f"{'first_ms':>9s} {'best_ms':>8s} {'kernel_ms':>9s} {'plain_ms':>8s} {'plain_max':>9s} {'read/nnz':>8s} "
          f"{'bfs_ms':>7s} {'cc/bfs':>7s}", flush=True)
    for name, make in graphs:
        g = make()
        labels = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        source = int(np.argmax(np.diff(g.offsets_to_host())))
        ea.bfs(ctx, g, source)  # warm: builds the hot-first copy
        bfs_ms = min(ea.bfs(ctx, g, source)[1].elapsed_ms for _ in range(3))
        want = None
        for rounds in ("default", "0"):
            if rounds == "0":
                os.environ["GRX_CC_SAMPLE_ROUNDS"] = "0"
            count, first, best, plain = measure(ctx, g, labels)
            os.environ.pop("GRX_CC_SAMPLE_ROUNDS", None)
            if want is None:
                want = labels.clone()
            assert torch.equal(labels, want)
            largest = int(torch.bincount(labels).max())
            print(f"{name:>16s} {rounds:>6s} {g.n_rows:9d} {g.nnz:11d} {count:10d} {largest:9d} "
                  f"{best.advance_launches:6d} {first.elapsed_ms:9.3f} {best.elapsed_ms:8.3f} "
                  f"{best.advance_kernel_ms:9.3f} {plain[0]:8.3f} {plain[-1]:9.3f} "
                  f"{best.edges_expanded / max(g.nnz, 1):8.4f} {bfs_ms:7.3f} {plain[0] / bfs_ms:7.2f}", flush=True)
        del g, labels, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
