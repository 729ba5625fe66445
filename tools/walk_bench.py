#!/usr/bin/env python3
"""grx_random_walk on symmetrised R-MAT as generated (scale 22, edge factor 16, seed 1, weight_seed 7):
2^20 walks of length 80 from seeded random starts among the vertices that have edges (the graph is
symmetric: no such walk meets a dead end), one process.

Per kind -- uniform, weighted, node2vec (p = 0.25, q = 4) and weighted node2vec -- the best of 3 whole
calls after a warm one: the call's time, the time of what the call builds first, steps and candidates
per second over the call and over the call less its builds.  A build is timed as a call of ONE walk
that needs it (one step for the prefix array of a weighted call, two steps for the sorted rows of a
node2vec call): everything but the build is then a launch of one lane.  Beside them the figure of
Context.gather_rate(mode 0) on the same graph, the ceiling of ONE random lookup; a uniform step needs
at least two dependent ones (the offset pair, then the column entry).  The second call of every kind
is compared with the first before a time is printed; kernels_ms is advance_kernel_ms of one more call
made with collect_kernel_time.  Nothing here is a pass condition.

    python tools/walk_bench.py [--out FILE] [scale [log2 walks [length]]]
    (default: 22 20 80, profiles/walk_bench.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def best_of_three(call):
    best, first = None, None
    for attempt in range(4):  # the first call warms
        out, st = call()
        if first is None:
            first = out.clone()
        else:
            assert torch.equal(out, first)
        if attempt and (best is None or st.elapsed_ms < best.elapsed_ms):
            best = st
    return best


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "walk_bench.txt")
    if args and args[0] == "--out":
        out, args = args[1], args[2:]
    scale, log_walks, length = ([int(x) for x in args] + [22, 20, 80][len(args):])[:3]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    ctx = ea.Context(0)
    g = ea.Graph.rmat(ctx, scale, 16, 1, 7)
    count = 1 << log_walks
    connected = np.flatnonzero(np.diff(g.offsets_to_host())).astype(np.int32)
    starts = connected[np.random.default_rng(80).integers(0, len(connected), count)]
    gather = max(ctx.gather_rate(g, mode=0) for _ in range(3))
    emit(f"rmat{scale} V {g.n_rows} nnz {g.nnz} walks {count} length {length} gather_rate_mode0 {gather / 1e9:.2f} G/s")
    emit(f"{'kind':>17s} {'call_ms':>9s} {'kernels_ms':>10s} {'build_ms':>9s} {'steps':>10s} {'candidates':>11s} {'Gsteps/s':>9s} "
         f"{'walking':>9s} {'Gcand/s':>9s} {'gather/step':>11s} {'full':>8s}")
    walks = torch.empty((count, length + 1), dtype=torch.int32, device="cuda")
    one = torch.empty((1, 3), dtype=torch.int32, device="cuda")
    for kind, kw in (("uniform", {}), ("weighted", {"weighted": True}), ("node2vec", {"p": 0.25, "q": 4.0}),
                     ("weighted node2vec", {"weighted": True, "p": 0.25, "q": 4.0})):
        st = best_of_three(lambda: ea.random_walk(ctx, g, starts, length, seed=1, walks=walks, **kw))
        _, timed = ea.random_walk(ctx, g, starts, length, seed=1, walks=walks,
                                  options=ea.Options(collect_kernel_time=True), **kw)
        steps = 2 if "p" in kw else 1
        build = best_of_three(lambda: ea.random_walk(ctx, g, starts[:1], steps, seed=1, walks=one[:, :steps + 1].contiguous(),
                                                     **kw))
        walking = max(st.elapsed_ms - (build.elapsed_ms if kw else 0.0), 1e-6)
        emit(f"{kind:>17s} {st.elapsed_ms:9.3f} {timed.advance_kernel_ms:10.3f} {build.elapsed_ms if kw else 0.0:9.3f} {st.edges_traversed:10d} "
             f"{st.edges_expanded:11d} {st.edges_traversed / st.elapsed_ms / 1e6:9.3f} "
             f"{st.edges_traversed / walking / 1e6:9.3f} {st.edges_expanded / walking / 1e6:9.3f} "
             f"{gather / (st.edges_traversed / walking * 1e3):11.1f} {st.vertices_reached:8d}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
