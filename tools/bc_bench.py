#!/usr/bin/env python3
"""grx_bc on the bench's graph (RMAT-22, edge factor 16, seeds 1 / 7), one source per call, over
the sources of tools/multi_source.py (vertex 0 and 15 seeded random non-isolated vertices): per
source the grx_bfs time, the single-source grx_bc time, their ratio and BC's TEPS
(edges_traversed / elapsed), best of 3 each; then the medians."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import essentials_amd as ea


def best(fn, repeats=3):
    out = None
    for _ in range(repeats):
        _, st = fn()
        if out is None or st.elapsed_ms < out.elapsed_ms:
            out = st
    return out


ctx = ea.Context(0)
g = ea.Graph.rmat(ctx, 22, 16, 1, 7)
deg = np.diff(g.offsets_to_host())
rng = np.random.default_rng(100)
sources = [0] + [int(x) for x in rng.choice(np.flatnonzero(deg > 0), 15)]
d = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
b = torch.empty(g.n_rows, dtype=torch.float32, device="cuda")
ea.bfs(ctx, g, sources[0], d)  # first use builds the hot-first copy
ea.bc(ctx, g, sources[0], b)
print(f"{'source':>8s} {'levels':>6s} {'bfs_ms':>8s} {'bc_ms':>8s} {'bc/bfs':>7s} {'bc_GTEPS':>9s}")
rows = []
for s in sources:
    bf = best(lambda: ea.bfs(ctx, g, s, d))
    bc = best(lambda: ea.bc(ctx, g, s, b))
    teps = bc.edges_traversed / (bc.elapsed_ms * 1e-3) / 1e9
    rows.append((bf.elapsed_ms, bc.elapsed_ms, bc.elapsed_ms / bf.elapsed_ms, teps))
    print(f"{s:8d} {bc.iterations:6d} {bf.elapsed_ms:8.3f} {bc.elapsed_ms:8.3f} {rows[-1][2]:7.2f} {teps:9.2f}",
          flush=True)
m = np.median(np.array(rows), axis=0)
print(f"{'median':>8s} {'':6s} {m[0]:8.3f} {m[1]:8.3f} {m[2]:7.2f} {m[3]:9.2f}")
