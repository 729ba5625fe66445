"""CPU checks of random walks' place in the product boundary (the header declares grx_random_walk,
the library exports it, the Python layer offers essentials_amd.random_walk), of the oracle the GPU
tests compare against (tests/walk_oracle.py) -- its hand-checked facts and the statistics of the
definition itself -- and of the header's selection functions, run on the host under sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from walk_oracle import (chi_square, csr, draw, mix64, mtx_csr, pick_uniform, pick_weighted, prefix, random_walk,
                         ratios, u24)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")
N = 2 ** 14
HUB = 38  # chesapeake's vertex of 33 entries


def test_header_declares_grx_random_walk():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_random_walk\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,"
                     r"\s*const\s+int32_t\s*\*\s*h_starts,\s*int32_t\s+n_starts,\s*int32_t\s+length,"
                     r"\s*uint64_t\s+seed,\s*int32_t\s+weighted,\s*float\s+p,\s*float\s+q,"
                     r"\s*int32_t\s*\*\s*d_walks,\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)


def test_header_states_the_biases():
    text = " ".join(open(HEADER).read().split())
    assert "d / 2^32 per entry" in text and "(63/64)^1024" in text and "GRX_WALK_MAX_ATTEMPTS" in text


def test_library_exports_grx_random_walk():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_random_walk")


def test_python_layer_offers_random_walk():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.random_walk) and "random_walk" in ea.__all__
    assert "grx_random_walk" in _SIGNATURES and len(_SIGNATURES["grx_random_walk"][1]) == 12


# ---- the oracle's hand-checked facts -----------------------------------------------------------------

def test_mix64_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0: its state advances by the constant mix64 adds
    assert mix64(0) == 0xE220A8397B1DCDAF
    assert mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert u24((1 << 64) - 1) == np.float32(1 - 2.0 ** -24) and u24((1 << 40) - 1) == 0


def test_oracle_on_the_directed_path():
    ap, aj, ax = csr(6, [(v, v + 1) for v in range(5)])
    for kw in ({}, {"weighted": True, "ax": ax}, {"p": 0.25, "q": 4.0}):
        got = random_walk(ap, aj, starts=[0, 3, 5], length=4, seed=9, **kw)
        assert got["walks"].tolist() == [[0, 1, 2, 3, 4], [3, 4, 5, -1, -1], [5, -1, -1, -1, -1]]
        assert got["iterations"] == 4 and got["full"] == 1 and got["steps"] == 6 and got["slots"] == [2, 2, 1, 1]
        # the only candidate of a row is two steps from prev: `far`, rejected 15 times in 16
        assert got["attempts"] > 6 if "p" in kw else got["attempts"] == 6
    assert random_walk(ap, aj, starts=[2], length=0)["walks"].tolist() == [[2]]
    none = random_walk(ap, aj, starts=[], length=3)
    assert none["walks"].shape == (0, 4) and none["iterations"] == 0 and none["slots"] == []


def test_p_q_one_is_the_first_order_walk():
    ap, aj, ax = mtx_csr(CHESAPEAKE)
    ax = (1 + np.arange(len(aj)) % 5).astype(np.float32)
    for weighted in (False, True):
        first = random_walk(ap, aj, ax, None, 12, seed=4, weighted=weighted)
        # the second-order machinery with every ratio 1: the same candidates, all accepted at once
        same = random_walk(ap, aj, ax, None, 12, seed=4, weighted=weighted, p=1.0, q=1.0, cap=1)
        assert (first["walks"] == same["walks"]).all() and first["attempts"] == first["steps"] == same["attempts"]
        assert ratios(1, 1) == (1, 1, 1)
        other = random_walk(ap, aj, ax, None, 12, seed=4, weighted=weighted, p=0.25, q=4.0)
        assert (first["walks"][:, :2] == other["walks"][:, :2]).all()      # step 1 has no prev
        assert (first["walks"] != other["walks"]).any() and other["attempts"] > other["steps"]


def test_ratios_are_float32_and_the_largest_is_one():
    assert ratios(0.25, 4) == (1, 0.25, 0.0625) and ratios(4, 0.25) == (0.0625, 0.25, 1)
    assert ratios(8, 8) == (0.125, 1, 0.125) and ratios(0.125, 8)[2] == np.float32(1 / 64)
    r = ratios(3, 0.7)
    assert all(x.dtype == np.float32 for x in r) and max(r) == 1


def test_prefix_blocks_and_the_weighted_pick():
    w = (np.arange(130) % 7).astype(np.float32)
    c = prefix(w)
    assert (c == np.cumsum(w.astype(np.float64))).all() and c[-1] == w.sum()   # small integers: exact
    assert pick_weighted(c, 0) == 1 and pick_weighted(c, (1 << 64) - 1) == 129
    # float32 sums that round: the bases are added block by block, not entry by entry
    w = np.full(200, 0.1, np.float32)
    c = prefix(w)
    assert c[63] == np.cumsum(w[:64], dtype=np.float32)[-1]
    assert c[64] == np.float32(c[63] + w[64])
    assert c[129] == np.float32(np.float32(c[63] + c[63]) + np.float32(w[128] + w[129]))
    assert c[129] != np.cumsum(w[:130], dtype=np.float32)[-1]  # ... which is not the plain running sum
    assert (np.diff(c) >= 0).all()


# ---- statistics of the definition: == then carries them to the GPU -----------------------------------
# Pearson's chi-square must lie below the 1 - 10^-6 quantile for its degrees of freedom.

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_uniform_step_is_uniform(seed):
    ap, aj, _ = mtx_csr(CHESAPEAKE)
    assert ap[HUB + 1] - ap[HUB] == 33
    got = random_walk(ap, aj, starts=[HUB] * N, length=1, seed=seed)["walks"][:, 1]
    row = aj[ap[HUB]:ap[HUB + 1]]
    stat, df = chi_square([(got == x).sum() for x in row], np.ones(33))
    print(f"uniform seed {seed}: chi-square {stat:.1f} at df {df}")
    assert df == 32 and stat < 85.23


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_weighted_step_follows_the_weights(seed):
    w = np.arange(130) % 7
    ap, aj, ax = csr(131, [(0, 1 + k) for k in range(130)], w)
    got = random_walk(ap, aj, ax, [0] * N, 1, seed=seed, weighted=True)["walks"][:, 1]
    counts = np.bincount(got - 1, minlength=130)
    assert counts[w == 0].sum() == 0  # an entry of weight 0 is never chosen
    stat, df = chi_square(counts, w)
    print(f"weighted seed {seed}: chi-square {stat:.1f} at df {df}")
    assert df == 110 and stat < 195.39


@pytest.mark.parametrize("seed", [1, 2])
def test_node2vec_second_step_has_the_node2vec_distribution(seed):
    """Two steps from the hub, the second conditioned on the first, against the exact transition
    probabilities: an entry's weight is ret back to the hub, adj to a neighbour of the hub, far else."""
    ap, aj, _ = mtx_csr(CHESAPEAKE)
    ret, adj, far = (float(x) for x in ratios(0.25, 4))
    got = random_walk(ap, aj, starts=[HUB] * N, length=2, seed=seed, p=0.25, q=4.0)
    walks = got["walks"]
    around = set(aj[ap[HUB]:ap[HUB + 1]].tolist())
    stat = df = 0
    for v in sorted(around):
        row = aj[ap[v]:ap[v + 1]]
        weight = [ret if x == HUB else adj if int(x) in around else far for x in row]
        second = walks[walks[:, 1] == v, 2]
        s, d = chi_square([(second == x).sum() for x in row], weight)
        stat, df = stat + s, df + d
    # attempts of a second step at v: geometric, with the mean ratio of row v as its success rate
    first = aj[ap[HUB]:ap[HUB + 1]]
    expected = np.mean([(ap[v + 1] - ap[v]) / sum(ret if x == HUB else adj if int(x) in around else far
                                                  for x in aj[ap[v]:ap[v + 1]]) for v in first])
    per_step = (got["attempts"] - N) / N
    print(f"node2vec seed {seed}: chi-square {stat:.1f} at df {df}, {per_step:.2f} attempts per second step "
          f"({expected:.2f} expected), {got['attempts'] / got['steps']:.2f} per step")
    assert df == 205 and stat < 316.0
    # a geometric count's deviation is below its mean: 5 % is more than 6 deviations of the mean of N
    assert got["steps"] == 2 * N and abs(per_step / expected - 1) < 0.05


# ---- the header's selection functions on the host ------------------------------------------------------

def expected_picks():
    """What tests/cpp/walk_pick_tests.cpp prints, from the oracle."""
    top = (1 << 64) - 1
    out = [f"draw {i} {draw(0x8000000000000005, i << 31, 3, 2 * i + 1)}" for i in range(4)]
    out.append(f"u24 0 {float(u24(top)):.9g}")
    out += [f"uniform 0 {pick_uniform(0xffffffff << 32, 70000)}", f"uniform 1 {pick_uniform(top, 70000)}",
            f"uniform 2 {pick_uniform(0xffffffff, 70000)}", f"uniform 3 {pick_uniform(0x80000000 << 32, 70001)}"]
    out += [f"uniform {4 + i} {pick_uniform(draw(7, i, 1, 0), 70000)}" for i in range(8)]
    tiny = np.float32(2.0 ** -149)
    c = prefix([0, 0, tiny, 0, 0])
    assert np.float32(u24(top) * c[-1]) == c[-1]  # the product rounds up to W
    out += [f"fallback 0 {pick_weighted(c, top)}", f"fallback 1 {pick_weighted(c, 0)}",
            f"fallback 2 {pick_weighted(c[:3], top)}"]

    def weighted_case(name, w, seed, draws):
        c = prefix(w)
        lines = [f"{name} {i} {pick_weighted(c, draw(seed, i, 1, 0))}" for i in range(draws)]
        return lines + [f"{name} lowest {pick_weighted(c, 0)}", f"{name} highest {pick_weighted(c, top)}"]

    out += weighted_case("zeros", [0, 0, 0, 1, 2, 0, 3, 0, 0], 11, 32)
    w = np.asarray([k % 7 + 0.125 * (k % 3) for k in range(65)], np.float32)
    out += weighted_case("row65", w, 12, 64)
    w[64] = 0
    out += weighted_case("row65z", w, 13, 16)
    row = [2, 5, 5, 9, 40]
    out += [f"class {i} {0 if x == 7 else 1 if x in row else 2}" for i, x in enumerate([0, 2, 3, 5, 9, 39, 40, 41, 7])]
    out += ["class 9 0", "class 10 2", "all picks printed"]
    return out


def test_selection_functions_on_the_host_under_sanitizers(tmp_path):
    # clang links the sanitizer runtime statically; g++ is told to
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    clang = rocm_clang if os.path.exists(rocm_clang) else shutil.which("clang++")
    gxx = shutil.which("g++")
    assert clang or gxx, "no C++ compiler"
    cmd = [clang] if clang else [gxx, "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "walk_pick_tests")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", "walk_pick_tests.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got, want = r.stdout.split("\n")[:-1], expected_picks()
    assert "fallback 0 2" in want and "fallback 1 2" in want and "fallback 2 2" in want and "zeros lowest 3" in want
    assert "zeros highest 6" in want and "uniform 0 69999" in want and "row65z highest 62" in want
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:8]
