#!/usr/bin/env python3
"""grx_sddmm and grx_spmm_values beside grx_spmm, which does the same row gather, and beside what a
caller had before them: (u[row] * v[col]).sum(-1) in torch.  A probe, not part of bench.py and not a
pass condition; reads nothing outside the repository.

Graphs: the symmetric R-MAT of scale 20 and the directed R-MAT of scale 22 with in-edges attached (edge
factor 16, seed 1, weight_seed 7, the benchmark's).  F in {16, 64, 128, 256}, features standard normal.
Per combination, after 2 warm-up rounds, 9 rounds of one call each, taking turns so that what else runs
on the machine meets all of them alike; medians with the smallest and largest in brackets:

  sddmm_ms       grx_sddmm, grx_stats.elapsed_ms (the whole call, its plan included)
  kern_ms        ... advance_kernel_ms (collect_kernel_time)
  spmm_ms        grx_spmm forward on the same handle and F
  sddmm/spmm     the ratio of the two medians
  torch_ms       (u[row] * v[col]).sum(-1) (device events around it), or "skipped" where its three
                 nnz x F temporaries do not fit in the free memory
  values_ms      grx_spmm_values forward with the handle's own values passed in
  valuesT_ms     ... transposed (n/a without in-edges: the call refuses), beside
  spmmT_ms       grx_spmm transposed
  gather_GB/s    nnz * 4 F bytes / kern_ms: the bytes of V the entries ask for, not the bytes that move

Before a time is printed, grx_sddmm is compared with the torch formulation on the first 2**20 entries
within the summation bound of F terms, and grx_spmm_values with the handle's own values is compared bit
for bit with grx_spmm.

    python tools/sddmm_probe.py [--out FILE] [--rounds N] [20 22 ...]   (default: 20 22, profiles/sddmm_probe.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = [16, 64, 128, 256]
WARM = 2
CHECKED = 1 << 20


def summary(values):
    v = np.sort(np.asarray(values, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def show(values):
    if not values:
        return "n/a"
    m, lo, hi = summary(values)
    return f"{m:.3f} ({lo:.3f}-{hi:.3f})"


def torch_scores(u, v, row, col):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    s = (u[row] * v[col]).sum(-1)
    b.record()
    b.synchronize()
    del s
    return a.elapsed_time(b)


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "sddmm_probe.txt")
    rounds = 9
    while args and args[0].startswith("--"):
        if args[0] == "--out":
            out = args[1]
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
    emit(f"copy_bandwidth_gbps {ctx.copy_bandwidth_gbps():.0f}; torch {torch.__version__}; "
         f"rounds {rounds} after {WARM}")
    emit(f"{'graph':>12s} {'V':>8s} {'nnz':>9s} {'F':>4s} {'sddmm_ms':>22s} {'kern_ms':>22s} {'spmm_ms':>22s} "
         f"{'sddmm/spmm':>10s} {'torch_ms':>25s} {'values_ms':>22s} {'valuesT_ms':>22s} {'spmmT_ms':>22s} "
         f"{'gather_GB/s':>11s}")
    for scale in scales:
        directed = scale >= 22
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=not directed)
        if directed:
            g.build_in_edges(ctx)
        name = f"rmat{scale}{'d+in' if directed else 'sym'}"
        ap, aj, aw = g.to_host()
        row = torch.repeat_interleave(torch.arange(g.n_rows), torch.from_numpy(np.diff(ap).astype(np.int64))).cuda()
        col = torch.from_numpy(aj[:g.nnz].astype(np.int64)).cuda()
        w = torch.from_numpy(np.ascontiguousarray(aw[:g.nnz], np.float32)).cuda()
        del ap, aj, aw
        rng = np.random.default_rng(scale)
        for F in FEATURES:
            u = torch.from_numpy(rng.standard_normal((g.n_rows, F)).astype(np.float32)).cuda()
            v = torch.from_numpy(rng.standard_normal((g.n_cols, F)).astype(np.float32)).cuda()
            s = torch.empty(g.nnz, dtype=torch.float32, device="cuda")
            y = torch.empty((g.n_rows, F), dtype=torch.float32, device="cuda")
            z = torch.empty((g.n_rows, F), dtype=torch.float32, device="cuda")
            # the same numbers two ways before anything is timed
            ea.sddmm(ctx, g, u, v, out=s)
            head = slice(0, min(CHECKED, g.nnz))
            a, b = u[row[head]].double(), v[col[head]].double()
            error = (s[head].double() - (a * b).sum(-1)).abs()
            assert bool((error <= 1.01 * (F + 1) * 2.0 ** -24 * (a.abs() * b.abs()).sum(-1)).all()), "sddmm disagrees"
            del a, b, error
            ea.spmm(ctx, g, v, y=y)
            ea.spmm(ctx, g, v, y=z, values=w)
            assert torch.equal(y.view(torch.int32), z.view(torch.int32)), "spmm_values differs from spmm"
            if directed:
                ea.spmm(ctx, g, v, y=y, transpose=True)
                ea.spmm(ctx, g, v, y=z, values=w, transpose=True)
                assert torch.equal(y.view(torch.int32), z.view(torch.int32)), "transposed spmm_values differs"
            # three nnz x F temporaries: the two gathers and their product
            free = torch.cuda.mem_get_info()[0]
            fits = 3 * g.nnz * F * 4 < 0.9 * free
            whole, kernels, product, dense, fwd, back, plain_back = [], [], [], [], [], [], []
            for r in range(WARM + rounds):
                _, st = ea.sddmm(ctx, g, u, v, out=s, options=opt)
                _, sp = ea.spmm(ctx, g, v, y=y)
                _, sf = ea.spmm(ctx, g, v, y=z, values=w)
                _, sb = ea.spmm(ctx, g, v, y=y, transpose=True)
                sv = ea.spmm(ctx, g, v, y=z, values=w, transpose=True)[1] if directed else None
                ms = None
                if fits:
                    try:
                        ms = torch_scores(u, v, row, col)
                    except torch.cuda.OutOfMemoryError:
                        fits = False
                        torch.cuda.empty_cache()
                if r >= WARM:
                    whole.append(st.elapsed_ms)
                    kernels.append(st.advance_kernel_ms)
                    product.append(sp.elapsed_ms)
                    fwd.append(sf.elapsed_ms)
                    plain_back.append(sb.elapsed_ms)
                    if sv is not None:
                        back.append(sv.elapsed_ms)
                    if ms is not None:
                        dense.append(ms)
            m_sddmm, m_kern, m_spmm = summary(whole)[0], summary(kernels)[0], summary(product)[0]
            emit(f"{name:>12s} {g.n_rows:8d} {g.nnz:9d} {F:4d} {show(whole):>22s} {show(kernels):>22s} "
                 f"{show(product):>22s} {m_sddmm / m_spmm:10.2f} {show(dense) if fits and dense else 'skipped':>25s} "
                 f"{show(fwd):>22s} {show(back):>22s} {show(plain_back):>22s} "
                 f"{g.nnz * 4.0 * F / m_kern / 1e6:11.0f}")
            del u, v, s, y, z
            torch.cuda.empty_cache()
        del g, row, col, w
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
