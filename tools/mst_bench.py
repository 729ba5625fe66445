#!/usr/bin/env python3
"""grx_mst on weighted symmetric RMAT-20 / 22 / 24 as generated (edge factor 16, seed 1, weight seed
7): chosen entries, total weight, Boruvka rounds, kernel launches, the first call, the best of 3
whole calls with and without the event pairs of collect_kernel_time, the kernels alone and
edges_expanded / nnz -- once with the row flags (GRX_MST_ROW_FLAGS=1, the default: a row whose
entries are all inside one component is not walked again) and once without (=0: every row in every
round).  Beside it, on the same handle in the same process: grx_cc as it runs by default, grx_cc
with GRX_CC_SAMPLE_ROUNDS=0 (a full edge walk: the floor for ONE round of the minimum search) and
grx_bfs from the vertex of largest degree, each best of 3 after a warm call; and the ratios
mst / (full-walk cc) and mst / (rounds x full-walk cc).

    python tools/mst_bench.py [scale ...]      (default: 20 22 24)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea


def measure(ctx, g, entries):
    timed = ea.Options(collect_kernel_time=True)
    out, weight, _, first = ea.mst(ctx, g, entries, options=timed)
    count = out.numel()
    best = None
    for _ in range(3):
        again, w, _, st = ea.mst(ctx, g, entries, options=timed)
        assert again.numel() == count and w == weight
        if best is None or st.elapsed_ms < best.elapsed_ms:
            best = st
    plain = sorted(ea.mst(ctx, g, entries)[3].elapsed_ms for _ in range(3))  # without the event pairs
    return count, weight, first, best, plain


def best_cc(ctx, g, labels):
    ea.cc(ctx, g, labels)
    return min(ea.cc(ctx, g, labels)[2].elapsed_ms for _ in range(3))


def main():
    scales = [int(x) for x in sys.argv[1:]] or [20, 22, 24]
    ctx = ea.Context(0)
    print(f"{'graph':>8s} {'flags':>5s} {'V':>9s} {'nnz':>11s} {'entries':>9s} {'weight':>12s} {'rounds':>6s} {'launch':>6s} "
          f"{'first_ms':>9s} {'best_ms':>8s} {'kernel_ms':>9s} {'plain_ms':>8s} {'plain_max':>9s} {'read/nnz':>8s} "
          f"{'cc_ms':>7s} {'ccfull_ms':>9s} {'bfs_ms':>7s} {'mst/ccfull':>10s} {'/rounds':>8s}", flush=True)
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        entries = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        labels = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        source = int(np.argmax(np.diff(g.offsets_to_host())))
        ea.bfs(ctx, g, source)  # warm: builds the hot-first copy
        bfs_ms = min(ea.bfs(ctx, g, source)[1].elapsed_ms for _ in range(3))
        cc_ms = best_cc(ctx, g, labels)
        os.environ["GRX_CC_SAMPLE_ROUNDS"] = "0"
        cc_full_ms = best_cc(ctx, g, labels)
        os.environ.pop("GRX_CC_SAMPLE_ROUNDS", None)
        want = None
        for flags in ("1", "0"):
            os.environ["GRX_MST_ROW_FLAGS"] = flags
            count, weight, first, best, plain = measure(ctx, g, entries)
            os.environ.pop("GRX_MST_ROW_FLAGS", None)
            if want is None:
                want = entries[:count].clone()
            assert torch.equal(entries[:count], want)
            print(f"{'rmat%d' % scale:>8s} {flags:>5s} {g.n_rows:9d} {g.nnz:11d} {count:9d} {weight:12.1f} "
                  f"{best.iterations:6d} {best.advance_launches:6d} {first.elapsed_ms:9.3f} {best.elapsed_ms:8.3f} "
                  f"{best.advance_kernel_ms:9.3f} {plain[0]:8.3f} {plain[-1]:9.3f} "
                  f"{best.edges_expanded / max(g.nnz, 1):8.4f} {cc_ms:7.3f} {cc_full_ms:9.3f} {bfs_ms:7.3f} "
                  f"{plain[0] / cc_full_ms:10.2f} {plain[0] / (best.iterations * cc_full_ms):8.2f}", flush=True)
        del g, entries, labels, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
