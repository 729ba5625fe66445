#!/usr/bin/env python3
"""grx_neighbor_sample on symmetrised R-MAT as generated (scale 22, edge factor 16, seed 1): 1024 seeds
drawn by a fixed numpy seed, one process.

Per fan-out list and per lane-group width (GRX_SAMPLE_GROUP 0 = the rule, 8, 64, 256): the best of 3
whole calls after a warm one (elapsed_ms), advance_kernel_ms of one more call made with
collect_kernel_time, the sampled edges, the candidates drawn, and sampled edges per second over both
times.  The second call of every configuration is compared with the first, and every width with the
rule, before a time is printed.  Beside them the one comparison with the memory system: sampled edges
times 16 bytes (4 of column read, 12 written) over the kernel time, against what
Context.gather_rate(mode 0) -- one random 4-byte lookup per entry -- moves on the same graph.  [25, 10]
and [15, 10, 5] are the mini-batch shapes; [64], [256] and [1024] reach the larger m that the widths
are chosen for.  Nothing here is a pass condition.

    python tools/sample_bench.py [--out FILE] [scale [seeds]]
    (default: 22 1024, profiles/sample_bench.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUTS = ([25, 10], [15, 10, 5], [64], [256], [1024])


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "sample_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scale, n_seeds = ([int(x) for x in args] + [22, 1024][len(args):])[:2]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    g = ea.Graph.rmat(ctx, scale, 16, 1)
    seeds = np.random.default_rng(25).choice(g.n_rows, n_seeds, replace=False).astype(np.int32)
    gather = max(ctx.gather_rate(g, mode=0) for _ in range(3))
    emit(f"rmat{scale} V {g.n_rows} nnz {g.nnz} seeds {n_seeds} gather_rate_mode0 {gather / 1e9:.2f} G/s "
         f"= {gather * 4 / 1e9:.1f} GB/s of gathered words")
    emit(f"{'fanouts':>12s} {'group':>5s} {'call_ms':>8s} {'kernels_ms':>10s} {'launches':>8s} {'nodes':>8s} {'edges':>9s} "
         f"{'candidates':>10s} {'Medges/s call':>13s} {'Medges/s kernels':>16s} {'GB/s kernels':>12s} {'of gather':>9s}")
    for fanouts in FANOUTS:
        rule = None
        for width in (0, 8, 64, 256):
            os.environ["GRX_SAMPLE_GROUP"] = str(width)
            best, first = None, None
            for attempt in range(4):  # the first call warms
                got, st = ea.neighbor_sample(ctx, g, seeds, fanouts, seed=1)
                if first is None:
                    first = got
                else:
                    assert torch.equal(got.nodes, first.nodes) and torch.equal(got.entries, first.entries)
                    assert torch.equal(got.src, first.src) and torch.equal(got.dst, first.dst)
                if attempt and (best is None or st.elapsed_ms < best.elapsed_ms):
                    best = st
            if rule is None:
                rule = first
            else:
                assert torch.equal(first.nodes, rule.nodes) and torch.equal(first.entries, rule.entries)
                assert torch.equal(first.dst, rule.dst)
            timed = min((ea.neighbor_sample(ctx, g, seeds, fanouts, seed=1,
                                            options=ea.Options(collect_kernel_time=True))[1] for _ in range(3)),
                        key=lambda s: s.advance_kernel_ms)
            edges = best.edges_traversed
            bytes_per_s = edges * 16 / (timed.advance_kernel_ms * 1e-3)
            emit(f"{str(fanouts):>12s} {width:5d} {best.elapsed_ms:8.3f} {timed.advance_kernel_ms:10.3f} "
                 f"{best.advance_launches:8d} {best.vertices_reached:8d} {edges:9d} {best.edges_expanded:10d} "
                 f"{edges / best.elapsed_ms / 1e3:13.1f} {edges / timed.advance_kernel_ms / 1e3:16.1f} "
                 f"{bytes_per_s / 1e9:12.2f} {bytes_per_s / (gather * 4):9.3f}")
        del os.environ["GRX_SAMPLE_GROUP"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
