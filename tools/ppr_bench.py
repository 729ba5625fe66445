#!/usr/bin/env python3
"""grx_ppr on symmetrised RMAT-16 / 20 / 22 as generated (edge factor 16, seed 1, weight_seed 7): 64
random distinct seeds (seeded), alpha 0.85, 20 iterations exactly (max_iterations 20, tol 0), one
process.

Per graph, the best of 3 whole calls after a warm one: ms per iteration of the whole call and of the
kernels alone (collect_kernel_time), the bytes of one iteration by the model
nnz * (8 + 4 L) + 3 * V * 4 L (every in-entry's source and weight and one L-column row of give; p read
and written and the next give written) over either time, beside Context.copy_bandwidth_gbps().  The
same with GRX_PPR_SEGMENT=2048, the one alternative measured.  The comparator: 64 times the
per-iteration time of ea.pagerank(direction_optimized=True, max_iterations=20) on the same handle,
what 64 unbatched power iterations of the library's fastest form would cost.  Below each graph: a
single seed (L = 16) the same way, where batching has nothing to share.  The batched rows are
compared with the single-seed row of their first seed before a time is printed.  Nothing here is a
pass condition.

    python tools/ppr_bench.py [--out FILE] [scale ...]    (default: 16 20 22, profiles/ppr_bench.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20


def best_of_three(call):
    best = None
    for attempt in range(4):  # the first call warms
        out, st = call()
        if attempt and (best is None or st.elapsed_ms < best.elapsed_ms):
            best = st
    return out, best


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "ppr_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scales = [int(x) for x in args] or [16, 20, 22]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    copy = ctx.copy_bandwidth_gbps()
    emit(f"copy_bandwidth_gbps {copy:.0f}")
    emit(f"{'graph':>7s} {'V':>8s} {'nnz':>10s} {'seeds':>5s} {'L':>3s} {'segment':>7s} {'call_ms':>9s} {'ms/it':>8s} "
         f"{'kern_ms/it':>10s} {'model_MB/it':>11s} {'GB/s':>7s} {'kern_GB/s':>9s} {'launch':>6s} {'pr_ms/it':>8s} "
         f"{'seeds*pr/it':>11s} {'unbatched/ppr':>13s}")
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        seeds = np.random.default_rng(64).choice(g.n_rows, 64, replace=False).astype(np.int32)
        opt = ea.Options(collect_kernel_time=True, max_iterations=T)
        _, pr = best_of_three(lambda: ea.pagerank(ctx, g, 0.85, 0.0, options=ea.Options(
            direction_optimized=True, max_iterations=T)))
        pr_ms = pr.elapsed_ms / max(pr.iterations, 1)
        single = None
        for count, segment in ((1, None), (64, None), (64, "2048")):
            L = 16 if count <= 16 else 32 if count <= 32 else 64
            if segment:
                os.environ["GRX_PPR_SEGMENT"] = segment
            p = torch.empty((count, g.n_rows), dtype=torch.float32, device="cuda")

            def call():
                ranks, info, st = ea.ppr(ctx, g, seeds[:count], tol=0.0, p=p, options=opt)
                return (ranks, info), st

            (p, info), st = best_of_three(call)
            os.environ.pop("GRX_PPR_SEGMENT", None)
            assert info["iterations"].tolist() == [T] * count and st.iterations == T
            if count == 1:
                single = p.clone()
            elif segment is None:
                assert torch.equal(p[0], single[0])
            model = g.nnz * (8 + 4 * L) + 3 * g.n_rows * 4 * L
            ms, kms = st.elapsed_ms / T, st.advance_kernel_ms / T
            emit(f"{'rmat%d' % scale:>7s} {g.n_rows:8d} {g.nnz:10d} {count:5d} {L:3d} {segment or '512':>7s} "
                 f"{st.elapsed_ms:9.3f} {ms:8.3f} {kms:10.3f} {model / 1e6:11.1f} {model / ms / 1e6:7.0f} "
                 f"{model / kms / 1e6:9.0f} {st.advance_launches:6d} {pr_ms:8.3f} {count * pr_ms:11.3f} "
                 f"{count * pr_ms / ms:13.2f}")
            del p
        del g, single
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
