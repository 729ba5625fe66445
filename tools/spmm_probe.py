#!/usr/bin/env python3
"""grx_spmm beside what a caller had before it: F calls of grx_spmv on the same handle.  A probe, not
part of bench.py and not a pass condition; reads nothing outside the repository.

Graphs: the symmetric R-MAT of scale 20 and the directed R-MAT of scale 22 with in-edges attached (edge
factor 16, seed 1, weight_seed 7, the benchmark's).  F in {16, 64, 128, 256}, forward and transposed,
features standard normal.  Per combination, after 2 warm-up rounds, 9 rounds of one grx_spmm call, one
grx_spmv call and (where it works) one torch.sparse.mm, taking turns so that what else runs on the
machine meets all three alike; medians with the smallest and largest in brackets:

  spmm_ms        grx_spmm, grx_stats.elapsed_ms (the whole call, its plan included)
  kern_ms        ... advance_kernel_ms (collect_kernel_time)
  F*spmv_ms      F times grx_spmv's elapsed_ms: F columns, one call each
  ratio          F*spmv_ms / spmm_ms (medians)
  torch_ms       torch.sparse.mm on the same CSR (device events around the call); informational
  X_MB           the size of the gathered matrix
  gather_GB/s    nnz * 4 F bytes / kern_ms: the bytes of X the entries ask for, not the bytes that move

Before a time is printed, column 0 of the product is compared bit for bit with the F = 1 call, and
with grx_spmv within the summation bound of a row.

    python tools/spmm_probe.py [--out FILE] [--rounds N] [20 22 ...]   (default: 20 22, profiles/spmm_probe.txt)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = [16, 64, 128, 256]
WARM = 2


def summary(values):
    v = np.sort(np.asarray(values, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def show(values):
    m, lo, hi = summary(values)
    return f"{m:.3f} ({lo:.3f}-{hi:.3f})"


def torch_csr(g, transpose):
    """The handle's CSR (or its transpose) as a torch sparse CSR tensor, or the reason there is none."""
    try:
        ap, aj, aw = g.to_host()
        offsets, columns = torch.from_numpy(ap.astype(np.int64)), torch.from_numpy(aj[:g.nnz].astype(np.int64))
        a = torch.sparse_csr_tensor(offsets, columns, torch.from_numpy(aw[:g.nnz]), size=(g.n_rows, g.n_cols)).cuda()
        if transpose:
            a = a.to_sparse_coo().t().coalesce().to_sparse_csr()
        return a, None
    except Exception as e:  # informational: the probe goes on without it
        return None, f"{type(e).__name__}: {str(e).splitlines()[0][:100]}"


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "spmm_probe.txt")
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
    emit(f"{'graph':>12s} {'V':>8s} {'nnz':>9s} {'dir':>3s} {'F':>4s} {'spmm_ms':>22s} {'kern_ms':>22s} "
         f"{'F*spmv_ms':>25s} {'ratio':>6s} {'torch_ms':>22s} {'spmm/torch':>10s} {'X_MB':>6s} {'gather_GB/s':>11s}")
    for scale in scales:
        directed = scale >= 22
        g = ea.Graph.rmat(ctx, scale, 16, 1, 7, symmetrize=not directed)
        if directed:
            g.build_in_edges(ctx)
        name = f"rmat{scale}{'d+in' if directed else 'sym'}"
        rng = np.random.default_rng(scale)
        for transpose in (False, True):
            sparse, why = torch_csr(g, transpose)
            if why:
                emit(f"# torch.sparse.mm unavailable on {name}{' transposed' if transpose else ''}: {why}")
            for F in FEATURES:
                x = torch.from_numpy(rng.standard_normal((g.n_cols, F)).astype(np.float32)).cuda()
                y = torch.empty((g.n_rows, F), dtype=torch.float32, device="cuda")
                column = x[:, 0].contiguous()
                v = torch.empty(g.n_rows, dtype=torch.float32, device="cuda")
                # the same product three ways before anything is timed
                ea.spmm(ctx, g, x, transpose=transpose, y=y)
                one, _ = ea.spmm(ctx, g, column[:, None], transpose=transpose)
                same = torch.equal(one[:, 0].view(torch.int32), y[:, 0].view(torch.int32))
                assert same, "column 0 differs from F = 1"
                ea.spmv(ctx, g, column, transpose=transpose, y=v)
                # two float32 sums of D terms each: |difference| <= 2 (D + 1) 2^-24 sum |terms|, and the
                # generator's weights are integers >= 1, so a row's weight sum bounds its D
                scale_of = ea.spmv(ctx, g, column.abs(), transpose=transpose)[0]
                terms = ea.spmv(ctx, g, torch.ones_like(column), transpose=transpose)[0]
                assert bool(((v - y[:, 0]).abs() <= 1.01 * 2.0 ** -23 * (terms + 1) * scale_of).all()), "spmv disagrees"
                del one, scale_of, terms
                whole, kernels, vector, dense = [], [], [], []
                torch_why = why
                for r in range(WARM + rounds):
                    _, st = ea.spmm(ctx, g, x, transpose=transpose, y=y, options=opt)
                    _, sv = ea.spmv(ctx, g, column, transpose=transpose, y=v)
                    ms = None
                    if sparse is not None and torch_why is None:
                        try:
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record()
                            z = torch.sparse.mm(sparse, x)
                            b.record()
                            b.synchronize()
                            ms = a.elapsed_time(b)
                            del z
                        except Exception as e:
                            torch_why = f"{type(e).__name__}: {str(e).splitlines()[0][:100]}"
                            emit(f"# torch.sparse.mm failed on {name} F={F}: {torch_why}")
                    if r >= WARM:
                        whole.append(st.elapsed_ms)
                        kernels.append(st.advance_kernel_ms)
                        vector.append(F * sv.elapsed_ms)
                        if ms is not None:
                            dense.append(ms)
                m_spmm, m_kern, m_vec = summary(whole)[0], summary(kernels)[0], summary(vector)[0]
                against = '%10.2f' % (m_spmm / summary(dense)[0]) if dense else 'n/a'
                emit(f"{name:>12s} {g.n_rows:8d} {g.nnz:9d} {'T' if transpose else 'N':>3s} {F:4d} {show(whole):>22s} "
                     f"{show(kernels):>22s} {show(vector):>25s} {m_vec / m_spmm:6.1f} "
                     f"{show(dense) if dense else 'n/a':>22s} {against:>10s} "
                     f"{g.n_cols * F * 4 / 1e6:6.0f} {g.nnz * 4.0 * F / m_kern / 1e6:11.0f}")
                del x, y, v, column
                torch.cuda.empty_cache()
            del sparse
        del g
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
