#!/usr/bin/env python3
"""grx_spgemm, A * A on symmetrised and directed R-MAT (edge factor 16, seed 1, unit weights): per
graph the products, nnz(C), the first call and the best of 5 after it (whole call, device events
inside the call), the kernels alone and their split into the bound, symbolic and numeric batches
(collect_kernel_time), and the rate in products per second.  No comparator: DESIGN.md, "Sparse
matrix product", says why.

    python tools/spgemm_bench.py [scale ...] [--largest]     (default: 14 16)

--largest: after the scales given, raise the scale of the symmetrised and of the directed graph
until the product is refused for having more than INT32_MAX entries, and measure the last scale
that fitted of each."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import essentials_amd as ea

HEAD = (f"{'graph':>12s} {'nnz(A)':>10s} {'products':>13s} {'nnz(C)':>12s} {'first_ms':>9s} {'best_ms':>9s} "
        f"{'kernel_ms':>9s} {'bound':>7s} {'symbolic':>8s} {'numeric':>8s} {'Gprod/s':>8s}")


def one(ctx, name, g):
    opts = ea.Options(collect_kernel_time=True)
    c, first = ea.spgemm(ctx, g, g, opts)
    nnz_c = c.nnz
    print(f"  {name}: first call {first.elapsed_ms:.3f} ms, {first.edges_expanded} products", flush=True)
    del c
    best = None
    for _ in range(5):
        c, st = ea.spgemm(ctx, g, g, opts)
        assert c.nnz == nnz_c
        del c
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    phases = [us / 1000.0 for us in best.frontier_slots]
    print(f"{name:>12s} {g.nnz:10d} {best.edges_expanded:13d} {nnz_c:12d} {first.elapsed_ms:9.3f} "
          f"{best.elapsed_ms:9.3f} {best.advance_kernel_ms:9.3f} {phases[0]:7.3f} {phases[1]:8.3f} {phases[2]:8.3f} "
          f"{best.edges_expanded / (best.elapsed_ms * 1e-3) / 1e9:8.2f}", flush=True)


def main():
    args = sys.argv[1:]
    largest = "--largest" in args
    scales = [int(x) for x in args if x != "--largest"] or [14, 16]
    ctx = ea.Context(0)
    print(HEAD, flush=True)
    for s in scales:
        for sym in (True, False):
            g = ea.Graph.rmat(ctx, s, 16, 1, 0, sym)
            one(ctx, f"rmat{s}{'s' if sym else 'd'}", g)
            del g
    for sym in (True, False) if largest else ():
        kind = "s" if sym else "d"
        s, fitted = max(scales) + 1, None
        while s <= 26:
            g = ea.Graph.rmat(ctx, s, 16, 1, 0, sym)
            try:
                c, st = ea.spgemm(ctx, g, g)
                fitted = s
                print(f"  rmat{s}{kind}: {c.nnz} entries from {st.edges_expanded} products, {st.elapsed_ms:.1f} ms",
                      flush=True)
                del c
            except ea.EngineError as e:
                if e.code != -3:
                    raise
                print(f"  rmat{s}{kind}: {e}", flush=True)
                break
            finally:
                del g
            s += 1
        if fitted is not None and fitted not in scales:
            g = ea.Graph.rmat(ctx, fitted, 16, 1, 0, sym)
            one(ctx, f"rmat{fitted}{kind}", g)
            del g


if __name__ == "__main__":
    main()
