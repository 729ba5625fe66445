#!/usr/bin/env python3
"""grx_scc on directed RMAT-20 / 22 / 24 (symmetrize=False, edge factor 16, seed 1), in-edges built
beforehand and that build timed separately: components, size of the largest, forward-backward
rounds, kernel launches, the best of 3 whole calls and the kernels alone (collect_kernel_time),
edges_expanded / nnz; beside them grx_cc (weak components, every row walked: the handle is directed)
and grx_bfs from the vertex of largest out-degree on the same handle in the same process, best of 3
after a warm call -- the honest yardsticks: nobody else has measured this call.

    python tools/scc_bench.py [scale ...]      (default: 20 22 24)"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea


def main():
    scales = [int(x) for x in sys.argv[1:]] or [20, 22, 24]
    ctx = ea.Context(0)
    timed = ea.Options(collect_kernel_time=True)
    print(f"{'graph':>16s} {'V':>9s} {'nnz':>11s} {'in_edges_ms':>11s} {'components':>10s} {'largest':>9s} {'rounds':>6s} "
          f"{'launch':>6s} {'best_ms':>8s} {'kernel_ms':>9s} {'read/nnz':>8s} {'cc_ms':>7s} {'weak':>9s} {'bfs_ms':>7s} "
          f"{'scc/cc':>7s} {'scc/bfs':>7s}", flush=True)
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 0, symmetrize=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.build_in_edges(ctx)  # returns when the transpose is complete
        in_edges_ms = (time.perf_counter() - t0) * 1e3
        labels = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        weak = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        source = int(np.argmax(np.diff(g.offsets_to_host())))
        ea.bfs(ctx, g, source)
        bfs_ms = min(ea.bfs(ctx, g, source)[1].elapsed_ms for _ in range(3))
        ea.cc(ctx, g, weak)
        cc = [ea.cc(ctx, g, weak) for _ in range(3)]
        cc_ms = min(st.elapsed_ms for _, _, st in cc)
        _, count, _ = ea.scc(ctx, g, labels, options=timed)
        want = labels.clone()
        best = None
        for _ in range(3):
            _, again, st = ea.scc(ctx, g, labels, options=timed)
            assert again == count and torch.equal(labels, want)
            if best is None or st.elapsed_ms < best.elapsed_ms:
                best = st
        largest = int(torch.bincount(labels).max())
        print(f"{'rmat%d.directed' % scale:>16s} {g.n_rows:9d} {g.nnz:11d} {in_edges_ms:11.3f} {count:10d} {largest:9d} "
              f"{best.iterations:6d} {best.advance_launches:6d} {best.elapsed_ms:8.3f} {best.advance_kernel_ms:9.3f} "
              f"{best.edges_expanded / max(g.nnz, 1):8.4f} {cc_ms:7.3f} {cc[0][1]:9d} {bfs_ms:7.3f} "
              f"{best.elapsed_ms / cc_ms:7.2f} {best.elapsed_ms / bfs_ms:7.2f}", flush=True)
        del g, labels, weak, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
