#!/usr/bin/env python3
"""grx_lpa on symmetrised RMAT-16 / 20 / 22 as generated (edge factor 16, seed 1, weight_seed 7), one
process.

Per graph, the best of 3 whole calls after a warm one: the call time, the sweeps, the communities and
the modularity; the time of ea.color on the same handle and its share of the call; the calls
stopped after 1, 2 and sweeps - 1 sweeps (max_iterations), whose differences are the second and the
last sweep; the first sweep as (call stopped after 1) - (colouring), which still holds the sort by
class, the initial labels and the two closing passes, so it is an upper bound; the first sweep's
entries per second from that bound (nnz entries decided, nnz more walked to set the dirty bytes)
beside Context.gather_rate of the same graph, the ceiling of one 4-byte gather per entry; the
entries the last sweep read; and the whole call again with GRX_LPA_ALL_ROWS=1 (no dirty bytes) and
with GRX_LPA_NARROW_EDGES=0 (a launch per class).  The labels of every variant are compared with
the first call's before a time is printed.  Nothing here is a pass condition.

    python tools/lpa_bench.py [--out FILE] [scale ...]    (default: 16 20 22, profiles/lpa_bench.txt)"""
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
    out = os.path.join(ROOT, "profiles", "lpa_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scales = [int(x) for x in args] or [16, 20, 22]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    emit(f"{'graph':>7s} {'V':>8s} {'nnz':>10s} {'colours':>7s} {'sweeps':>6s} {'communities':>11s} {'Q':>7s} "
         f"{'call_ms':>9s} {'color_ms':>8s} {'color%':>6s} {'launch':>6s} {'first_ms<=':>10s} {'second_ms':>9s} "
         f"{'last_ms':>8s} {'last_read':>10s} {'first_Ge/s>=':>12s} {'gather_Ge/s':>11s} {'all_rows_ms':>11s} "
         f"{'no_narrow_ms':>12s} {'no_narrow_launch':>16s}")
    for scale in scales:
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
        labels = torch.empty(g.n_rows, dtype=torch.int32, device="cuda")
        other = torch.empty_like(labels)
        _, colours, color_st = best_of_three(lambda: ea.color(ctx, g))
        _, count, q, st = best_of_three(lambda: ea.lpa(ctx, g, labels))
        sweeps = st.iterations

        def stopped_after(t):
            return best_of_three(lambda: ea.lpa(ctx, g, other, options=ea.Options(max_iterations=t)))[-1]

        t1, t2 = stopped_after(1), stopped_after(2)
        before_last = stopped_after(sweeps - 1) if sweeps > 2 else t1
        first_ms = t1.elapsed_ms - color_st.elapsed_ms
        last_ms = st.elapsed_ms - before_last.elapsed_ms
        last_read = st.edges_expanded - before_last.edges_expanded
        gather = ctx.gather_rate(g, 0)
        variants = []
        for hook in ("GRX_LPA_ALL_ROWS", "GRX_LPA_NARROW_EDGES"):
            os.environ[hook] = "1" if hook == "GRX_LPA_ALL_ROWS" else "0"
            _, count2, q2, st2 = best_of_three(lambda: ea.lpa(ctx, g, other))
            os.environ.pop(hook)
            assert torch.equal(other, labels) and (count2, q2, st2.iterations) == (count, q, sweeps)
            variants.append(st2)
        emit(f"{'rmat%d' % scale:>7s} {g.n_rows:8d} {g.nnz:10d} {colours:7d} {sweeps:6d} {count:11d} {q:7.4f} "
             f"{st.elapsed_ms:9.3f} {color_st.elapsed_ms:8.3f} {100 * color_st.elapsed_ms / st.elapsed_ms:6.1f} "
             f"{st.advance_launches:6d} {first_ms:10.3f} {t2.elapsed_ms - t1.elapsed_ms:9.3f} {last_ms:8.3f} "
             f"{last_read:10d} {2 * g.nnz / first_ms / 1e6:12.2f} {gather / 1e9:11.2f} {variants[0].elapsed_ms:11.3f} "
             f"{variants[1].elapsed_ms:12.3f} {variants[1].advance_launches:16d}")
        emit(f"        changes per sweep {st.frontier_slots}")
        del g, labels, other
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
