"""CPU checks of Louvain's place in the product boundary (the header declares grx_louvain, the
library exports it, the Python layer offers essentials_amd.louvain) and of the numpy oracle the GPU
tests compare against (tests/louvain_oracle.py): the vectorised `communities` equals the sequential
definition, row order does not matter, the score rises strictly over kept sweeps and survives
aggregation, the phases coarsen, a committed case takes the undo branch, a planted partition is
recovered, and answers written by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from louvain_oracle import (UNDO_EDGES, communities, csr, level_graph, modularity_parts, mtx_csr, planted, sequential,
                            simple_csr)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")

def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_louvain\s*\(", text)
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", open(HEADER).read())


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_louvain")


def test_python_layer_offers_louvain():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.louvain) and "louvain" in ea.__all__
    assert "grx_louvain" in _SIGNATURES and len(_SIGNATURES["grx_louvain"][1]) == 8


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows (the generator of test_lpa_abi.py)."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = np.concatenate([e, e[rng.integers(0, m, 80)], np.stack([np.arange(0, n, 5)] * 2, 1)])
    ap, aj = csr(n, e)
    for u in range(n):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    return ap, aj


def _same(a, b):
    assert a[0].dtype == np.int32 and a[0].tolist() == b[0].tolist()
    assert a[1:] == b[1:]


def _graphs():
    return (mtx_csr(CHESAPEAKE), _random_multigraph(), simple_csr(*_random_multigraph()))


def _coarsens(fine, coarse):
    """Every community of `fine` lies inside one community of `coarse`."""
    return len(np.unique(np.stack([fine, coarse], 1), axis=0)) == len(np.unique(fine))


def test_vectorised_equals_sequential():
    for ap, aj in _graphs():
        want = sequential(ap, aj)
        _same(communities(ap, aj), want)
        label, count, q, levels, kept, shapes = want
        n = len(ap) - 1
        assert (label <= np.arange(n)).all() and (label[label] == label).all()
        assert count == len(np.unique(label)) and kept.count(0) == levels == len(shapes) and kept[-1] == 0
        assert shapes[0] == (n, len(aj)) and q == modularity_parts(ap, aj, label)[2]


def test_row_order_does_not_matter():
    ap, aj = _random_multigraph(seed=9)
    want = communities(ap, aj)
    rng = np.random.default_rng(1)
    aj = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    _same(communities(ap, aj), want)


def test_per_phase_invariants():
    for ap, aj in _graphs() + (planted()[:2],):
        n, e = len(ap) - 1, len(aj)
        trace = []
        full = communities(ap, aj, trace=trace)
        levels = full[3]
        assert len(trace) == levels
        # N rises strictly over kept sweeps, and the next phase starts from the score the last one reached
        scores = [s for record in trace for s in record["scores"]]
        for record, after in zip(trace, trace[1:]):
            assert all(b > a for a, b in zip(record["scores"], record["scores"][1:]))
            assert after["scores"][0] == record["scores"][-1]
        assert len(trace[-1]["scores"]) == 1 and scores[-1] >= scores[0]
        # E and N survive aggregation: the level graph's weight is E, and its singleton partition scores N
        for t in range(1, levels):
            lap, laj, law = level_graph(ap, aj, t)
            assert int(law.sum()) == e and (len(lap) - 1, len(laj)) == full[5][t]
            row = np.repeat(np.arange(len(lap) - 1), np.diff(lap))
            k = np.bincount(row, weights=law, minlength=len(lap) - 1).astype(np.int64)
            inside = int(law[row == laj].sum())
            assert inside * e - sum(int(x) * int(x) for x in k) == trace[t]["scores"][0]
            dense = np.zeros((len(lap) - 1,) * 2, np.int64)
            dense[row, laj] = law
            assert (dense == dense.T).all() and (np.diff(laj)[np.diff(row) == 0] > 0).all()
        # the partition after t + 1 phases coarsens the one after t, and Q does not fall
        cuts = [communities(ap, aj, max_phases=t) for t in range(1, levels + 1)]
        _same(cuts[-1][:3], full[:3])
        singles = modularity_parts(ap, aj, np.arange(n))[2]
        qs = [singles] + [c[2] for c in cuts]
        for t, cut in enumerate(cuts):
            i, s, q = modularity_parts(ap, aj, cut[0])
            assert q == cut[2] and i * e - s == trace[t]["scores"][-1]
            if t:
                assert _coarsens(cuts[t - 1][0], cut[0]) and cut[1] <= cuts[t - 1][1]
        assert all(b >= a for a, b in zip(qs, qs[1:]))
        assert full[2] > singles if any(full[4]) else full[2] == singles


def test_the_undo_path_by_hand():
    ap, aj = csr(8, np.asarray(UNDO_EDGES, np.int64))
    for run in (sequential, communities):
        trace = []
        label, count, q, levels, kept, shapes = run(ap, aj, trace=trace)
        assert levels == 2 and kept == [6, 0, 0] and shapes[0] == (8, 34) and shapes[1][0] == 2
        assert trace[0]["undone"] and not trace[1]["undone"] and len(trace[0]["scores"]) == 2
        assert count == 2 and len(np.unique(label)) == 2


def test_planted_partition():
    ap, aj, block = planted()
    label, count, q, levels, kept, shapes = communities(ap, aj)
    print(f"planted: communities {count} levels {levels} Q {q!r} kept {kept} shapes {shapes}")
    assert count == 20 and (label == block * 25).all()


def _nx_graph(nx, ap, aj):
    n = len(ap) - 1
    src = np.repeat(np.arange(n), np.diff(ap))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
    return G


def test_against_networkx():
    nx = pytest.importorskip("networkx")
    for name, (ap, aj) in (("chesapeake", mtx_csr(CHESAPEAKE)), ("planted", planted()[:2]),
                           ("planted p_out 0.03", planted(p_out=0.03)[:2])):
        label, _, q, _, _, _ = communities(ap, aj)
        G = _nx_graph(nx, ap, aj)
        best = max(nx.community.modularity(G, nx.community.louvain_communities(G, seed=seed)) for seed in range(5))
        print(f"{name}: oracle Q {q:.6f}, networkx best of 5 {best:.6f}, gap {q - best:+.6f}")  # recorded, not asserted
        groups = [set(np.flatnonzero(label == l).tolist()) for l in np.unique(label)]
        assert abs(q - nx.community.modularity(G, groups)) < 1e-12


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


def test_two_cliques_and_a_bridge_by_hand():
    ap, aj = csr(10, np.asarray(_clique(0, 5) + _clique(5, 5) + [(4, 5)], np.int64))
    for run in (sequential, communities):
        label, count, q, levels, kept, shapes = run(ap, aj)
        assert label.tolist() == [0] * 5 + [5] * 5 and count == 2 and q == 40 / 42 - 0.5
        assert kept.count(0) == levels and shapes[-1] == (2, 4)


def test_isolated_vertices_self_loops_and_nothing_by_hand():
    # 0, 2 and 5 are isolated, 1 has only a self loop: each keeps its own label
    ap, aj = csr(6, np.asarray([(1, 1), (3, 4)], np.int64))
    for run in (sequential, communities):
        label, count, q, levels, kept, shapes = run(ap, aj)
        assert label.tolist() == [0, 1, 2, 3, 3, 5] and count == 5 and levels == 2 and kept == [1, 0, 0]
        assert shapes == [(6, 4), (5, 2)] and q == modularity_parts(ap, aj, label)[2] == 1.0 - 8 / 16
    ap, aj = csr(4, np.zeros((0, 2), np.int64))
    _same(sequential(ap, aj), communities(ap, aj))
    assert communities(ap, aj)[0].tolist() == [0, 1, 2, 3] and communities(ap, aj)[1:] == (4, 0.0, 1, [0], [(4, 0)])
    ap, aj = csr(0, np.zeros((0, 2), np.int64))
    _same(sequential(ap, aj), communities(ap, aj))
    assert communities(ap, aj)[1:] == (0, 0.0, 0, [], [])


def test_one_phase_is_a_prefix_of_the_full_run():
    ap, aj = _random_multigraph(seed=11)
    full = communities(ap, aj)
    assert full[3] > 2
    part = communities(ap, aj, max_phases=1)
    _same(part, sequential(ap, aj, max_phases=1))
    ends = [t for t, moved in enumerate(full[4]) if moved == 0]
    assert part[3] == 1 and part[4] == full[4][:ends[0] + 1] and part[5] == full[5][:1]
    assert _coarsens(part[0], full[0])
