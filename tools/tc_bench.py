#!/usr/bin/env python3
"""grx_tc on symmetric RMAT-20 / 22 / 24 (edge factor 16, seeds 1 / 7) and chesapeake: per graph
T, the first call and the best of 3 (whole call), the counting kernels (collect_kernel_time)
against the preprocessing (the rest of the call), the rate in simple edges per second, and --
when oracle/_ref/libgrx_ref_clients.so has refc_tc -- the unchanged tc.hxx on the deduplicated,
row-sorted copy of the same graph, timed by the ms it returns (best of 3).

    python tools/tc_bench.py [scale ...]      (default: 20 22 24)"""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import essentials_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libgrx_ref_clients.so")


def ref_tc_lib():
    if not os.path.exists(REF):
        return None
    L = C.CDLL(REF)
    if not hasattr(L, "refc_tc"):
        return None
    L.refc_tc.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_ulonglong), C.POINTER(C.c_float)]
    return L


def dedup_sorted(g):
    """unique(row * n + col) on the device, then bincount / cumsum for the offsets."""
    ap, aj, _ = g.to_host()
    n = g.n_rows
    ap_d = torch.from_numpy(ap.astype("int64")).cuda()
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), ap_d[1:] - ap_d[:-1])
    key = torch.unique(row * n + torch.from_numpy(aj.astype("int64")).cuda())
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.bincount(key // n, minlength=n), 0)
    return off.int().contiguous(), (key % n).int().contiguous()


def main():
    scales = [int(x) for x in sys.argv[1:]] or [20, 22, 24]
    ctx = ea.Context(0)
    L = ref_tc_lib()
    graphs = [("chesapeake", lambda: ea.Graph.from_mtx(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")))]
    graphs += [(f"rmat{s}", lambda s=s: ea.Graph.rmat(ctx, s, 16, 1, 7)) for s in scales]
    print(f"{'graph':>10s} {'nnz':>11s} {'simple_E':>11s} {'T':>13s} {'first_ms':>9s} {'best_ms':>8s} "
          f"{'count_ms':>9s} {'prep_ms':>8s} {'GE/s':>7s} {'probes':>13s} {'ref_ms':>8s} {'ref/grx':>7s}",
          flush=True)
    for name, make in graphs:
        g = make()
        counts = torch.empty(g.n_rows, dtype=torch.int64, device="cuda")
        opts = ea.Options(collect_kernel_time=True)
        t0 = time.perf_counter()
        _, T, first = ea.tc(ctx, g, counts, options=opts)
        first_wall = (time.perf_counter() - t0) * 1e3
        best = None
        for _ in range(3):
            _, T2, st = ea.tc(ctx, g, counts, options=opts)
            assert T2 == T
            if best is None or st.elapsed_ms < best.elapsed_ms:
                best = st
        rate = best.edges_traversed / (best.elapsed_ms * 1e-3) / 1e9
        ref_ms = float("nan")
        if L is not None:
            off, col = dedup_sorted(g)
            val = torch.ones(col.numel(), dtype=torch.float32, device="cuda")
            rc = torch.zeros(g.n_rows, dtype=torch.int32, device="cuda")
            ms, tot = C.c_float(), C.c_ulonglong()
            for _ in range(3):
                rc.zero_()  # tc.hxx adds into the per-vertex counts it is given
                torch.cuda.synchronize()
                assert L.refc_tc(g.n_rows, col.numel(), off.data_ptr(), col.data_ptr(), val.data_ptr(), rc.data_ptr(),
                                 tot, ms) == 0
                ref_ms = ms.value if ref_ms != ref_ms else min(ref_ms, ms.value)
            torch.cuda.synchronize()
            if tot.value != 3 * T:
                print(f"  note: tc.hxx total {tot.value} != 3 T = {3 * T}", flush=True)
            del off, col, val, rc
        print(f"{name:>10s} {g.nnz:11d} {best.edges_traversed:11d} {T:13d} {first.elapsed_ms:9.3f} "
              f"{best.elapsed_ms:8.3f} {best.advance_kernel_ms:9.3f} {best.elapsed_ms - best.advance_kernel_ms:8.3f} "
              f"{rate:7.2f} {best.edges_expanded:13d} {ref_ms:8.3f} {ref_ms / best.elapsed_ms:7.2f}"
              f"   (first call wall {first_wall:.1f} ms)", flush=True)
        del g, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
