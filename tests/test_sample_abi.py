"""CPU checks of neighbour sampling's place in the product boundary (the header declares
grx_neighbor_sample, the library exports it, the Python layer offers essentials_amd.neighbor_sample),
of the oracle the GPU tests compare against (tests/sample_oracle.py) -- its hand-checked facts and the
statistics of the definition itself -- and of the header's scalar functions, run on the host under
sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sample_oracle import (ALL, EXCLUDE, INCLUDE, attempt_bound, candidate, csr, mtx_csr, neighbor_sample,
                           sample_plan, sample_row)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
N = 2 ** 14
HUB = 38  # chesapeake's vertex of 33 entries


def test_header_declares_grx_neighbor_sample():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_neighbor_sample\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,"
                     r"\s*const\s+int32_t\s*\*\s*h_seeds,\s*int32_t\s+n_seeds,"
                     r"\s*const\s+int32_t\s*\*\s*h_fanouts,\s*int32_t\s+n_hops,\s*uint64_t\s+seed,"
                     r"\s*int32_t\s*\*\s*d_nodes,\s*int64_t\s+node_capacity,"
                     r"\s*int32_t\s*\*\s*d_src,\s*int32_t\s*\*\s*d_dst,\s*int32_t\s*\*\s*d_entry,"
                     r"\s*int64_t\s+edge_capacity,\s*int64_t\s*\*\s*h_node_offsets,"
                     r"\s*int64_t\s*\*\s*h_edge_offsets,\s*const\s+grx_options\s*\*\s*opt,"
                     r"\s*grx_stats\s*\*\s*stats\s*\)", text)


def test_header_states_the_definition():
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    for words in ("64 m + 1024", "GRX_SAMPLE_GROUP", "first m distinct values", "ascending position",
                  "in ascending vertex id", "min(distinct seeds + edges, V)", "Two host hand-offs per hop"):
        assert words in text, words


def test_library_exports_grx_neighbor_sample():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_neighbor_sample")


def test_python_layer_offers_neighbor_sample():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.neighbor_sample) and "neighbor_sample" in ea.__all__ and "NeighborSample" in ea.__all__
    assert "grx_neighbor_sample" in _SIGNATURES and len(_SIGNATURES["grx_neighbor_sample"][1]) == 17
    assert "nodes[src]" in ea.neighbor_sample.__doc__ and "torch.stack([dst, src])" in ea.neighbor_sample.__doc__


# ---- the oracle's hand-checked facts -----------------------------------------------------------------

PATH = csr(6, [(v, v + 1) for v in range(5)])
STAR = csr(6, [(0, 1 + k) for k in range(5)])


def test_plan_at_its_boundaries():
    for k in (1, 8, 9, 64, 65, 1024):
        assert sample_plan(k, k) == (ALL, 0) and sample_plan(k - 1, k) == (ALL, 0) and sample_plan(0, k) == (ALL, 0)
        assert sample_plan(2 * k, k) == (INCLUDE, k) and sample_plan(2 * k + 1, k) == (INCLUDE, k)
        if k > 1:
            assert sample_plan(k + 1, k) == (EXCLUDE, 1) and sample_plan(2 * k - 1, k) == (EXCLUDE, k - 1)
    assert sample_plan(2, 1) == (INCLUDE, 1)  # k + 1 == 2k
    assert sample_plan(70000, -1) == (ALL, 0) and sample_plan(0, -1) == (ALL, 0)
    for d in range(1, 80):
        for k in range(1, 80):
            mode, m = sample_plan(d, k)
            assert 2 * m <= d and (m > 0) == (mode != ALL)
    assert attempt_bound(1) == 1088 and attempt_bound(1024) == 66560


def test_oracle_on_the_directed_path():
    ap, aj, _ = PATH
    got = neighbor_sample(ap, aj, [0], [1, 1, 1], seed=0)
    assert got["nodes"].tolist() == [0, 1, 2, 3] and got["node_offsets"] == [0, 1, 2, 3, 4]
    assert got["edge_offsets"] == [0, 1, 2, 3] and got["src"].tolist() == [0, 1, 2] and got["dst"].tolist() == [1, 2, 3]
    assert got["entries"].tolist() == [0, 1, 2]
    assert got["attempts"] == 0 and got["expanded"] == 3  # all-rows: no draws, their lengths are counted
    assert got["iterations"] == 3 and got["slots"] == [1, 1, 1]


def test_oracle_on_the_star():
    ap, aj, _ = STAR
    for seed in range(8):
        got = neighbor_sample(ap, aj, [0], [2], seed=seed)     # include: m = 2
        leaves = got["nodes"][1:].tolist()
        assert sample_plan(5, 2) == (INCLUDE, 2) and len(leaves) == 2 and leaves == sorted(leaves)
        assert got["entries"].tolist() == [x - 1 for x in leaves] and got["src"].tolist() == [0, 0]
        assert got["dst"].tolist() == [1, 2] and got["attempts"] >= 2 and got["expanded"] == got["attempts"]
        other = neighbor_sample(ap, aj, [0], [3], seed=seed)   # exclude: the same two are left out
        assert sample_plan(5, 3) == (EXCLUDE, 2) and other["attempts"] == got["attempts"]
        assert sorted(other["nodes"][1:].tolist() + leaves) == [1, 2, 3, 4, 5]
        assert other["entries"].tolist() == sorted(other["entries"].tolist()) and len(other["entries"]) == 3
    positions, A = sample_row(3, 1, 0, 4, 2)  # 2k == d is include
    assert sample_plan(4, 2) == (INCLUDE, 2) and len(positions) == 2 and A >= 2
    assert sample_row(3, 1, 0, 5, -1) == ([0, 1, 2, 3, 4], 0) and sample_row(3, 1, 0, 0, 4) == ([], 0)


def test_sample_row_follows_the_candidates_literally():
    for seed, hop, v, d, k in ((1, 1, 7, 33, 8), (2, 3, 2 ** 31 + 5, 33, 17), (2 ** 63 + 5, 64, 0, 40, 20)):
        positions, A = sample_row(seed, hop, v, d, k)
        xs = [candidate(seed, v, hop, a, d) for a in range(A)]
        mode, m = sample_plan(d, k)
        assert len(set(xs)) == m and len(set(xs[:-1])) == m - 1  # A is the smallest
        chosen = set(xs) if mode == INCLUDE else set(range(d)) - set(xs)
        assert positions == sorted(chosen) and len(positions) == k


def test_duplicate_seeds_are_dropped_and_the_first_is_kept():
    ap, aj, _ = PATH
    got = neighbor_sample(ap, aj, [3, 1, 3, 1, 0], [1], seed=0)
    assert got["nodes"].tolist() == [3, 1, 0, 2, 4] and got["node_offsets"] == [0, 3, 5]
    assert got["src"].tolist() == [0, 1, 2] and got["dst"].tolist() == [4, 3, 1]  # 3 -> 4, 1 -> 2, 0 -> 1


def test_a_dead_end_leaves_later_offsets_repeating():
    ap, aj, _ = PATH
    got = neighbor_sample(ap, aj, [4], [1, 1, 1], seed=0)
    assert got["nodes"].tolist() == [4, 5] and got["node_offsets"] == [0, 1, 2, 2, 2]
    assert got["edge_offsets"] == [0, 1, 1, 1] and got["slots"] == [1, 1, 0] and got["iterations"] == 2


def test_two_rows_naming_one_vertex_give_one_node_and_the_level_is_ascending():
    ap, aj, _ = csr(6, [(0, 5), (0, 2), (1, 5), (1, 4), (5, 0)])
    got = neighbor_sample(ap, aj, [1, 0], [-1, -1], seed=0)
    assert got["nodes"].tolist() == [1, 0, 2, 4, 5] and got["node_offsets"] == [0, 2, 5, 5]
    assert got["src"].tolist() == [0, 0, 1, 1, 4] and got["dst"].tolist() == [4, 3, 4, 2, 1]
    assert got["entries"].tolist() == [2, 3, 0, 1, 4] and got["slots"] == [2, 3] and got["expanded"] == 5


# ---- statistics of the definition: == then carries them to the GPU -----------------------------------

@pytest.mark.parametrize("k", [1, 8, 16, 17, 32])
@pytest.mark.parametrize("seed0", [1, 2, 3])
def test_every_k_subset_is_equally_likely(seed0, k):
    """N samples of k of the d = 33 positions of one row, O_i the times position i was chosen.
    One sample's indicator vector X has E X_i = k/d, Var X_i = (k/d)(1 - k/d) and, for i != j,
    Cov(X_i, X_j) = k(k-1)/(d(d-1)) - (k/d)^2 = -(k/d)(d-k)/(d(d-1)): the covariance matrix is
    c1 (I - J/d) with c1 = (k/d)(d-k)/(d-1) (diagonal c1 (d-1)/d, off-diagonal -c1/d; J all ones).
    The N samples are independent, so O has covariance c (I - J/d) with c = (Nk/d)(d-k)/(d-1).
    I - J/d projects onto the d - 1 dimensions orthogonal to the ones vector, where O - E O lives
    (the O_i sum to Nk), so |O - E O|^2 / c is asymptotically chi-square with d - 1 = 32 degrees of
    freedom, and |O - E O|^2 / c = sum((O_i - Nk/d)^2 / (Nk/d)) * (d-1)/(d-k).  It must lie below
    85.23, the 1 - 10^-6 quantile at df = 32.  Attempts per sample: the i-th new position takes a
    geometric number of attempts of mean d/(d-i), so the mean of A is sum_{i<m} d/(d-i) (exactly 1 at
    m = 1); A's deviation is below its mean, so 5 % is far more than 6 deviations of the mean of N."""
    ap, aj, _ = mtx_csr(CHESAPEAKE)
    d = int(ap[HUB + 1] - ap[HUB])
    assert d == 33
    counts, attempts = np.zeros(d, np.int64), 0
    for s in range(N):
        positions, A = sample_row(seed0 * 1000003 + s, 1, HUB, d, k)
        assert len(positions) == k
        counts[positions] += 1
        attempts += A
    expected = N * k / d
    stat = float(((counts - expected) ** 2 / expected).sum()) * (d - 1) / (d - k)
    mode, m = sample_plan(d, k)
    predicted = sum(d / (d - i) for i in range(m))
    print(f"k {k} seed0 {seed0}: statistic {stat:.1f} at df {d - 1}, {attempts / N:.3f} attempts per sample "
          f"({predicted:.3f} predicted, m = {m})")
    assert stat < 85.23
    if m == 1:
        assert attempts == N
    else:
        assert abs(attempts / N / predicted - 1) < 0.05


# ---- the header's scalar functions on the host ---------------------------------------------------------

def expected_facts():
    """What tests/cpp/sample_pick_tests.cpp prints, from the oracle."""
    out = []
    for k in (1, 8, 9, 64, 65, 1024):
        for d in (k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, 0):
            out.append("plan %d %d %d %d" % ((d, k) + sample_plan(d, k)))
    out += ["plan %d -1 %d %d" % ((d,) + sample_plan(d, -1)) for d in (0, 1, 5, 70000, 2147483647)]
    out += [f"bound {m} {attempt_bound(m)}" for m in (1, 2, 16, 512, 1024)]
    rows = [(0, 0, 1, 33), (7, 38, 1, 33), (7, 38, 2, 33), (0x8000000000000005, 38, 64, 70000),
            (1, 1 << 31, 3, 2049), (1, (1 << 31) + 5, 3, 2049), (1, 0xffffffff, 1, 2147483647),
            (1, (1 << 40) + 3, 1, 17)]
    for i, (seed, v, hop, d) in enumerate(rows):
        out += [f"candidate {i} {a} {candidate(seed, v, hop, a, d)}" for a in (0, 1, 2, 3, 1023, 66559)]
    return out + ["all facts printed"]


def test_scalar_functions_on_the_host_under_sanitizers(tmp_path):
    # clang links the sanitizer runtime statically; g++ is told to
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    clang = rocm_clang if os.path.exists(rocm_clang) else shutil.which("clang++")
    gxx = shutil.which("g++")
    assert clang or gxx, "no C++ compiler"
    cmd = [clang] if clang else [gxx, "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "sample_pick_tests")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", "sample_pick_tests.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got, want = r.stdout.split("\n")[:-1], expected_facts()
    assert "plan 2 1 1 1" in want and "plan 17 9 2 8" in want and "plan 2049 1024 1 1024" in want
    assert "plan 1024 1024 0 0" in want and "bound 1024 66560" in want
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:8]
