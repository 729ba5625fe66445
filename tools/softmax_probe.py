#!/usr/bin/env python3
"""grx_edge_softmax and grx_edge_softmax_backward beside grx_spmv on the same handle, which walks the same
rows and reads the column ids and a gathered operand besides, and beside what a caller had before them:
the torch composition over an nnz-long row index.  A probe, not part of bench.py and not a pass
condition; reads nothing outside the repository.

Graphs: the symmetric R-MAT of scale 20 and the directed R-MAT of scale 22 with in-edges attached (edge
factor 16, seed 1, weight_seed 7, the benchmark's).  Scores uniform in [-16, 16).  After 2 warm-up rounds,
9 rounds of one call each, taking turns so that what else runs on the machine meets all of them alike;
medians with the smallest and largest in brackets:

  fwd_ms / fwd_kern    grx_edge_softmax by row: grx_stats.elapsed_ms (the whole call, its plan included)
                       and advance_kernel_ms (collect_kernel_time)
  bwd_ms / bwd_kern    grx_edge_softmax_backward by row
  col_ms / col_kern    grx_edge_softmax by column (n/a without in-edges: the call refuses)
  fwd_GB/s, bwd_GB/s   the model's bytes over the kernel time: 8 nnz + 4 n forward, 12 nnz + 4 n backward
  of_copy              fwd_GB/s over Context.copy_bandwidth_gbps
  spmv_ms              grx_spmv forward on the same handle
  torch_ms             repeat_interleave'd row ids (made once, outside the time), then
                       scatter_reduce(amax), exp, index_add, division (device events around them)
  err/bound            the worst |out - float64| / float64 over all entries, divided by
                       tests/softmax_oracle.forward_bound for the entry's group (its length and spread)

Before a time is printed the forward result by row, and by column where it runs, is compared with the
float64 composition in torch entry by entry within that bound.

    python tools/softmax_probe.py [--out FILE] [--rounds N] [20 22 ...]   (default: 20 22, profiles/softmax_probe.txt)"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import essentials_amd as ea
from softmax_oracle import forward_bound

WARM = 2


def summary(values):
    v = np.sort(np.asarray(values, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def show(values):
    if not values:
        return "n/a"
    m, lo, hi = summary(values)
    return f"{m:.3f} ({lo:.3f}-{hi:.3f})"


def composition(s, index, n):
    """The softmax of s over the entries that share index[e], as torch offers it."""
    m = torch.full((n,), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, index, s, "amax")
    p = torch.exp(s - m[index])
    total = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, index, p)
    return p / total[index]


def torch_ms(s, index, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = composition(s, index, n)
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def used_of_the_bound(out, s, index, n):
    """max over entries of (relative error against float64) / forward_bound(group length, group spread)."""
    s64 = s.double()
    want = composition(s64, index, n)
    length = torch.zeros(n, dtype=torch.float64, device=s.device).index_add_(0, index, torch.ones_like(s64))
    top = torch.full((n,), float("-inf"), dtype=torch.float64, device=s.device).scatter_reduce(0, index, s64, "amax")
    low = torch.full((n,), float("inf"), dtype=torch.float64, device=s.device).scatter_reduce(0, index, s64, "amin")
    bound = forward_bound(length, torch.where(length > 0, top - low, torch.zeros_like(top)))[index]
    ratio = (out.double() - want).abs() / want / bound
    return float(ratio.max())


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "softmax_probe.txt")
    rounds = 9
    while args and args[0].startswith("--"):
        if args[0] == "--out":
            out_path = args[1]
        elif args[0] == "--rounds":
            rounds = int(args[1]) | 1
        else:
            raise SystemExit(__doc__)
        args = args[2:]
    scales = [int(x) for x in args] or [20, 22]
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    assert torch.cuda.is_available(), "the probe needs the GPU"
    ctx = ea.Context(0)
    opt = ea.Options(collect_kernel_time=True)
    copy = ctx.copy_bandwidth_gbps()
    emit(f"copy_bandwidth_gbps {copy:.0f}; torch {torch.__version__}; rounds {rounds} after {WARM}")
    emit(f"{'graph':>12s} {'V':>8s} {'nnz':>9s} {'fwd_ms':>22s} {'fwd_kern':>22s} {'bwd_ms':>22s} {'bwd_kern':>22s} "
         f"{'col_ms':>22s} {'col_kern':>22s} {'fwd_GB/s':>8s} {'of_copy':>7s} {'bwd_GB/s':>8s} {'spmv_ms':>22s} "
         f"{'torch_ms':>25s} {'err/bound':>9s} {'col err/bound':>13s}")
    for scale in scales:
        directed = scale >= 22
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=not directed)
        if directed:
            g.build_in_edges(ctx)
        name = f"rmat{scale}{'d+in' if directed else 'sym'}"
        ap, aj, _ = g.to_host()
        n, nnz = g.n_rows, g.nnz
        row = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(ap).astype(np.int64))).cuda()
        col = torch.from_numpy(aj[:nnz].astype(np.int64)).cuda()
        del ap, aj
        gen = torch.Generator(device="cuda").manual_seed(scale)
        s = torch.rand(nnz, dtype=torch.float32, device="cuda", generator=gen) * 32 - 16
        t = torch.rand(nnz, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
        x = torch.rand(g.n_cols, dtype=torch.float32, device="cuda", generator=gen)
        a = torch.empty(nnz, dtype=torch.float32, device="cuda")
        d = torch.empty(nnz, dtype=torch.float32, device="cuda")
        c = torch.empty(nnz, dtype=torch.float32, device="cuda")
        y = torch.empty(n, dtype=torch.float32, device="cuda")
        # the same numbers two ways before anything is timed
        ea.edge_softmax(ctx, g, s, out=a)
        used = used_of_the_bound(a, s, row, n)
        assert used <= 1.0, f"edge_softmax by row uses {used:.3f} of its bound"
        used_col = None
        if directed:
            ea.edge_softmax(ctx, g, s, by="column", out=c)
            used_col = used_of_the_bound(c, s, col, g.n_cols)
            assert used_col <= 1.0, f"edge_softmax by column uses {used_col:.3f} of its bound"
        torch.cuda.empty_cache()
        fwd, fwd_k, bwd, bwd_k, by_col, by_col_k, product, dense = [], [], [], [], [], [], [], []
        for r in range(WARM + rounds):
            _, sf = ea.edge_softmax(ctx, g, s, out=a, options=opt)
            _, sb = ea.edge_softmax_backward(ctx, g, a, t, out=d, options=opt)
            sc = ea.edge_softmax(ctx, g, s, by="column", out=c, options=opt)[1] if directed else None
            _, sp = ea.spmv(ctx, g, x, y=y)
            ms = torch_ms(s, row, n)
            if r >= WARM:
                fwd.append(sf.elapsed_ms)
                fwd_k.append(sf.advance_kernel_ms)
                bwd.append(sb.elapsed_ms)
                bwd_k.append(sb.advance_kernel_ms)
                product.append(sp.elapsed_ms)
                dense.append(ms)
                if sc is not None:
                    by_col.append(sc.elapsed_ms)
                    by_col_k.append(sc.advance_kernel_ms)
        fwd_rate = (8.0 * nnz + 4.0 * n) / summary(fwd_k)[0] / 1e6
        bwd_rate = (12.0 * nnz + 4.0 * n) / summary(bwd_k)[0] / 1e6
        emit(f"{name:>12s} {n:8d} {nnz:9d} {show(fwd):>22s} {show(fwd_k):>22s} {show(bwd):>22s} {show(bwd_k):>22s} "
             f"{show(by_col):>22s} {show(by_col_k):>22s} {fwd_rate:8.0f} {fwd_rate / copy:7.2f} {bwd_rate:8.0f} "
             f"{show(product):>22s} {show(dense):>25s} {used:9.3f} "
             f"{'n/a' if used_col is None else format(used_col, '.3f'):>13s}")
        del g, row, col, s, t, x, a, d, c, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
