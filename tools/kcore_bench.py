#!/usr/bin/env python3
"""grx_kcore on chesapeake and symmetric RMAT-20 / 22 / 24 (edge factor 16, seeds 1 / 7), each as
generated (a multigraph) and as Graph.simple: degeneracy, levels, kernel launches, the first call
and the best of 3 (whole call), the peeling kernels (collect_kernel_time) against the rest of the
call, nnz / elapsed, and for scale one grx_bfs on the same handle.

Second part, the reference's formulation on the same graph: the simple R-MAT of scale 16 and 18 is
written as a 'pattern symmetric' Matrix Market file into a temporary directory, the reference's
own harness oracle/_ref/ref_kcore (the unchanged kcore.hxx on this engine's operators) runs on it
as a child process, and essentials_amd.kcore is timed on Graph.from_mtx of the same file.  Skipped
when that binary was not built.

    python tools/kcore_bench.py [scale ...]      (default: 20 22 24)"""
import os
import re
import subprocess
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_kcore")


def measure(ctx, g):
    cores = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
    opts = ea.Options(collect_kernel_time=True)
    _, d, first = ea.kcore(ctx, g, cores, options=opts)
    best = None
    for _ in range(3):
        _, d2, st = ea.kcore(ctx, g, cores, options=opts)
        assert d2 == d and st.edges_expanded == g.nnz
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    plain = min(ea.kcore(ctx, g, cores)[2].elapsed_ms for _ in range(3))  # without the event pairs
    return d, first, best, plain


def write_mtx(path, ap, aj):
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap.astype(np.int64)))
    low = row > aj
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate pattern symmetric\n")
        f.write(f"{n} {n} {int(low.sum())}\n")
        np.savetxt(f, np.stack([row[low] + 1, aj[low].astype(np.int64) + 1], 1), fmt="%d %d")


def main():
    scales = [int(x) for x in sys.argv[1:]] or [20, 22, 24]
    ctx = ea.Context(0)
    graphs = [("chesapeake", lambda: ea.Graph.from_mtx(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")))]
    graphs += [(f"rmat{s}", lambda s=s: ea.Graph.rmat(ctx, s, 16, 1, 7)) for s in scales]
    print(f"{'graph':>16s} {'V':>9s} {'nnz':>11s} {'degen':>6s} {'levels':>6s} {'launch':>6s} {'first_ms':>9s} "
          f"{'best_ms':>8s} {'kernel_ms':>9s} {'rest_ms':>8s} {'plain_ms':>8s} {'GE/s':>6s} {'bfs_ms':>7s} {'kcore/bfs':>9s}",
          flush=True)
    for name, make in graphs:
        g = make()
        for label, h in ((name, g), (name + ".simple", g.simple(ctx))):
            d, first, best, plain = measure(ctx, h)
            source = int(np.argmax(np.diff(h.offsets_to_host())))
            bfs_ms = min(ea.bfs(ctx, h, source)[1].elapsed_ms for _ in range(3))
            print(f"{label:>16s} {h.n_rows:9d} {h.nnz:11d} {d:6d} {best.iterations:6d} {best.advance_launches:6d} "
                  f"{first.elapsed_ms:9.3f} {best.elapsed_ms:8.3f} {best.advance_kernel_ms:9.3f} "
                  f"{best.elapsed_ms - best.advance_kernel_ms:8.3f} {plain:8.3f} {h.nnz / (plain * 1e-3) / 1e9:6.2f} "
                  f"{bfs_ms:7.3f} {plain / bfs_ms:9.2f}", flush=True)
            del h
        del g
        torch.cuda.empty_cache()

    if not os.path.exists(REF):
        print("oracle/_ref/ref_kcore was not built: the reference's formulation is not measured", flush=True)
        return
    print(f"\n{'file':>16s} {'V':>9s} {'nnz':>11s} {'degen':>6s} {'ref_kcore GPU ms':>17s} {'grx_kcore ms':>13s} {'ref/grx':>8s}",
          flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for s in (16, 18):
            ap, aj, _ = ea.Graph.rmat(ctx, s, 16, 1, 7).simple(ctx).to_host()
            path = os.path.join(tmp, f"rmat{s}_simple.mtx")
            write_mtx(path, ap, aj)
            g = ea.Graph.from_mtx(path)
            d, _, _, plain = measure(ctx, g)
            t0 = time.perf_counter()
            r = subprocess.run([REF, path], capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            assert r.returncode == 0 and "Number of errors : 0" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
            ref_ms = float(re.search(r"GPU Elapsed Time : ([0-9.eE+-]+)", r.stdout).group(1))
            print(f"{'rmat%d.simple' % s:>16s} {g.n_rows:9d} {g.nnz:11d} {d:6d} {ref_ms:17.3f} {plain:13.3f} "
                  f"{ref_ms / plain:8.1f}   (harness wall {wall:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
