#!/usr/bin/env python3
"""grx_color on chesapeake and symmetric RMAT-20 / 22 / 24 (edge factor 16, seeds 1 / 7), each as
generated (a multigraph) and as Graph.simple: colours, iterations (the depth of the priority DAG),
kernel launches, the first call and the best of 3 (whole call), the kernels (collect_kernel_time)
against the rest of the call, nnz / elapsed, and grx_kcore on the same handle.

Second part, the reference's formulation on the same graph: the simple R-MAT of scale 16 and 18 is
written as a 'pattern symmetric' Matrix Market file into a temporary directory, the reference's
own harness oracle/_ref/ref_color (the unchanged color.hxx on this engine's operators) runs on it
as a child process, and essentials_amd.color is timed on Graph.from_mtx of the same file.  Skipped
when that binary was not built.

    python tools/color_bench.py [scale ...]      (default: 20 22 24)"""
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
REF = os.path.join(ROOT, "oracle", "_ref", "ref_color")


def measure(ctx, g):
    colors = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
    opts = ea.Options(collect_kernel_time=True)
    _, count, first = ea.color(ctx, g, colors, options=opts)
    best = None
    for _ in range(3):
        _, count2, st = ea.color(ctx, g, colors, options=opts)
        assert count2 == count and st.edges_expanded == 2 * g.nnz
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    plain = min(ea.color(ctx, g, colors)[2].elapsed_ms for _ in range(3))  # without the event pairs
    return count, first, best, plain


def write_mtx(path, ap, aj):
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap.astype(np.int64)))
    aj = aj[: len(row)]
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
    print(f"{'graph':>16s} {'V':>9s} {'nnz':>11s} {'colours':>7s} {'iters':>6s} {'launch':>6s} {'first_ms':>9s} "
          f"{'best_ms':>8s} {'kernel_ms':>9s} {'rest_ms':>8s} {'plain_ms':>8s} {'GE/s':>6s} {'kcore_ms':>8s} "
          f"{'color/kcore':>11s}", flush=True)
    for name, make in graphs:
        g = make()
        for label, h in ((name, g), (name + ".simple", g.simple(ctx))):
            count, first, best, plain = measure(ctx, h)
            kcore_ms = min(ea.kcore(ctx, h)[2].elapsed_ms for _ in range(3))
            print(f"{label:>16s} {h.n_rows:9d} {h.nnz:11d} {count:7d} {best.iterations:6d} {best.advance_launches:6d} "
                  f"{first.elapsed_ms:9.3f} {best.elapsed_ms:8.3f} {best.advance_kernel_ms:9.3f} "
                  f"{best.elapsed_ms - best.advance_kernel_ms:8.3f} {plain:8.3f} {h.nnz / (plain * 1e-3) / 1e9:6.2f} "
                  f"{kcore_ms:8.3f} {plain / kcore_ms:11.2f}", flush=True)
            del h
        del g
        torch.cuda.empty_cache()

    if not os.path.exists(REF):
        print("oracle/_ref/ref_color was not built: the reference's formulation is not measured", flush=True)
        return
    print(f"\n{'file':>16s} {'V':>9s} {'nnz':>11s} {'ref colours':>11s} {'ref_color GPU ms':>17s} {'grx colours':>11s} "
          f"{'grx_color ms':>13s} {'ref/grx':>8s}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for s in (16, 18):
            ap, aj, _ = ea.Graph.rmat(ctx, s, 16, 1, 7).simple(ctx).to_host()
            path = os.path.join(tmp, f"rmat{s}_simple.mtx")
            write_mtx(path, ap, aj)
            g = ea.Graph.from_mtx(path)
            count, _, _, plain = measure(ctx, g)
            t0 = time.perf_counter()
            r = subprocess.run([REF, path], capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            assert r.returncode == 0 and "Number of errors : 0" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
            ref_ms = float(re.search(r"GPU Elapsed Time : ([0-9.eE+-]+)", r.stdout).group(1))
            ref_colors = int(re.search(r"Number of colors : (\d+)", r.stdout).group(1))
            print(f"{'rmat%d.simple' % s:>16s} {g.n_rows:9d} {g.nnz:11d} {ref_colors:11d} {ref_ms:17.3f} {count:11d} "
                  f"{plain:13.3f} {ref_ms / plain:8.1f}   (harness wall {wall:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
