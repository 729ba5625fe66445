"""CPU checks of graph colouring's place in the product boundary (the header declares grx_color, the
library exports it, the Python layer offers essentials_amd.color) and of the numpy oracle the GPU
tests compare against (tests/color_oracle.py): the vectorised `colouring` equals the sequential
definition `greedy`, and both are proper colourings within the bounds the contract states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from color_oracle import (KNOWN, colouring, csr, fmix32, greedy, is_proper, keys, known_csr, mtx_csr, predecessors,
                          simple_csr)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_color\s*\(", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_color")


def test_python_layer_offers_color():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.color) and "color" in ea.__all__
    assert "grx_color" in _SIGNATURES


def test_fmix32_is_injective_and_matches_the_scalar_recipe():
    h = fmix32(np.arange(1 << 20))
    assert len(np.unique(h)) == 1 << 20 and int(h.max()) < 1 << 32

    def scalar(x):
        x ^= x >> 16
        x = (x * 0x85ebca6b) & 0xffffffff
        x ^= x >> 13
        x = (x * 0xc2b2ae35) & 0xffffffff
        return x ^ (x >> 16)

    for v in (0, 1, 2, 12345, (1 << 20) - 1, 0x7fffffff, 0xffffffff):
        assert int(fmix32(v)) == scalar(v)
    assert int(fmix32(0)) == 0 and int(fmix32(1)) == 0x514e28b7


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def _check(ap, aj):
    """colouring == greedy; proper; color[v] <= distinct predecessors <= deg(v)."""
    want = greedy(ap, aj)
    got, count, depth = colouring(ap, aj)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    n = len(ap) - 1
    assert count == (int(want.max()) + 1 if n else 0)
    assert is_proper(ap, aj, got)
    pred = predecessors(ap, aj)
    assert (got <= pred).all() and (pred <= np.diff(np.asarray(ap, np.int64))).all()
    assert (depth >= 1) == (n > 0) and depth <= n
    return got, count, depth


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_oracle_known_answers(name):
    ap, aj, want = known_csr(name)
    got, count, depth = _check(ap, aj)
    assert got.tolist() == want.tolist()
    assert count == (int(want.max()) + 1 if len(want) else 0)


def test_oracle_on_chesapeake_and_a_multigraph():
    for ap, aj in (mtx_csr(CHESAPEAKE), _random_multigraph(), simple_csr(*_random_multigraph(seed=6))):
        _, count, depth = _check(ap, aj)
        assert count > 2 and depth > 2


def test_depth_is_the_longest_chain_of_predecessors():
    ap, aj = _random_multigraph(seed=8)
    key = keys(ap)
    n = len(ap) - 1
    depth = np.zeros(n, np.int64)
    for v in np.argsort(key)[::-1]:
        row = aj[ap[v]:ap[v + 1]]
        before = row[(row != v) & (key[row] > key[v])]
        depth[v] = 1 + (depth[before].max() if len(before) else 0)
    assert colouring(ap, aj)[2] == depth.max()


def test_oracle_ignores_row_order_and_counts_repeats_in_the_degree():
    ap, aj = _random_multigraph(seed=9)
    want = colouring(ap, aj)
    rng = np.random.default_rng(1)
    aj = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    got = colouring(ap, aj)
    assert (got[0] == want[0]).all() and got[1:] == want[1:]
    # the simple graph under it has other degrees, hence another order and another answer
    simple = colouring(*simple_csr(ap, aj))[0]
    assert (simple != want[0]).any()


def test_against_networkx():
    nx = pytest.importorskip("networkx")
    for ap, aj in (mtx_csr(CHESAPEAKE), simple_csr(*_random_multigraph())):
        n = len(ap) - 1
        G = nx.Graph()
        G.add_nodes_from(range(n))
        src = np.repeat(np.arange(n), np.diff(ap))
        G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
        color, count, _ = colouring(ap, aj)
        assert count <= max(d for _, d in G.degree()) + 1
        assert all(color[a] != color[b] for a, b in G.edges() if a != b)


def test_clique_star_and_ring_by_hand():
    for n in (3, 17, 70):
        ap, aj = csr(n, [(a, b) for a in range(n) for b in range(a + 1, n)])
        color, count, depth = _check(ap, aj)
        assert count == n == depth and sorted(color.tolist()) == list(range(n))
    for hub in (0, 40):
        ap, aj = csr(41, [(hub, i) for i in range(41) if i != hub])
        color, count, depth = _check(ap, aj)
        assert color[hub] == 0 and (np.delete(color, hub) == 1).all() and count == 2 == depth
    ap, aj = csr(64, [(i, (i + 1) % 64) for i in range(64)])
    color, count, _ = _check(ap, aj)
    assert 2 <= count <= 3
