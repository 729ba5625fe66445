#!/usr/bin/env python3
"""grx_louvain on symmetrised RMAT-16 / 20 / 22 as generated (edge factor 16, seed 1, weight_seed 7),
one process.

Per graph, the best of 3 whole calls after a warm one: the call time, the levels, the sweeps, the
communities and Q; grx_lpa's Q and time on the same handle; and the call's time split three ways:
`color_ms` is ea.color on the handle (the colouring of level 0; the colourings of the coarse levels
are in the rest), `moves_ms` is the call's advance_kernel_ms under collect_kernel_time (the sort by
class, the sweeps with their score passes and hand-offs, the final naming), and `aggregation_ms` is
what remains of that timed call: the contractions, the coarse colourings and the host between
batches.  The labels of the timed call are compared with the first call's before a time is printed.
Nothing here is a pass condition.

    python tools/louvain_bench.py [--out FILE] [scale ...]    (default: 16 20 22, profiles/louvain_bench.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def best_of_three(call):
    best = None
    for attempt in range(4):  # the first call warms
        out = call()
        if attempt and (best is None or out[-1].elapsed_ms < best[-1].elapsed_ms):
            best = out
    return best


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "louvain_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scales = [int(x) for x in args] or [16, 20, 22]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    emit(f"{'graph':>7s} {'V':>8s} {'nnz':>10s} {'levels':>6s} {'sweeps':>6s} {'communities':>11s} {'Q':>8s} "
         f"{'call_ms':>9s} {'launch':>6s} {'lpa_Q':>8s} {'lpa_communities':>15s} {'lpa_ms':>8s} {'color_ms':>8s} "
         f"{'moves_ms':>8s} {'aggregation_ms':>14s}")
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        labels = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        other = torch.empty_like(labels)
        _, count, q, levels, st = best_of_three(lambda: ea.louvain(ctx, g, labels))
        _, lpa_count, lpa_q, lpa_st = best_of_three(lambda: ea.lpa(ctx, g, other))
        _, _, color_st = best_of_three(lambda: ea.color(ctx, g))
        _, count2, q2, levels2, timed = best_of_three(
            lambda: ea.louvain(ctx, g, other, options=ea.Options(collect_kernel_time=True)))
        assert torch.equal(other, labels) and (count2, q2, levels2, timed.iterations) == (count, q, levels, st.iterations)
        rest = timed.elapsed_ms - color_st.elapsed_ms - timed.advance_kernel_ms
        emit(f"{'rmat%d' % scale:>7s} {g.n_rows:8d} {g.nnz:10d} {levels:6d} {st.iterations:6d} {count:11d} {q:8.5f} "
             f"{st.elapsed_ms:9.3f} {st.advance_launches:6d} {lpa_q:8.5f} {lpa_count:15d} {lpa_st.elapsed_ms:8.3f} "
             f"{color_st.elapsed_ms:8.3f} {timed.advance_kernel_ms:8.3f} {rest:14.3f}")
        emit(f"        moves kept per sweep {st.frontier_slots}")
        del g, labels, other
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
