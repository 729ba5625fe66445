"""CPU checks of community detection's place in the product boundary (the header declares grx_lpa
and grx_modularity, the library exports them, the Python layer offers essentials_amd.lpa and
essentials_amd.modularity) and of the numpy oracle the GPU tests compare against
(tests/lpa_oracle.py): the vectorised `communities` equals the sequential definition, the dirty rule
changes nothing, every changing sweep raises the same-label entries, and answers written by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lpa_oracle import (communities, csr, inside_entries, modularity_parts, mtx_csr, sequential, simple_csr)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_lpa\s*\(", text)
    assert re.search(r"\bint\s+grx_modularity\s*\(", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_lpa") and hasattr(lib, "grx_modularity")


def test_python_layer_offers_lpa_and_modularity():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.lpa) and "lpa" in ea.__all__
    assert callable(ea.modularity) and "modularity" in ea.__all__
    assert "grx_lpa" in _SIGNATURES and "grx_modularity" in _SIGNATURES


def _random_multigraph(seed=4, n=60, m=400):
    """Symmetric CSR with repeated edges, self loops and shuffled rows."""
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


def test_vectorised_equals_sequential():
    for ap, aj in _graphs():
        want = sequential(ap, aj)
        _same(communities(ap, aj), want)
        label, count, sweeps, changes, _ = want
        n = len(ap) - 1
        assert (label <= np.arange(n)).all() and (label[label] == label).all()
        assert count == len(np.unique(label)) and sweeps == len(changes) and changes[-1] == 0


def test_the_dirty_rule_changes_neither_labels_nor_sweeps():
    for ap, aj in _graphs():
        dirty, every = sequential(ap, aj), sequential(ap, aj, all_rows=True)
        _same(dirty[:4], every[:4])
        _same(communities(ap, aj, all_rows=True), every)
        # every vertex decides every sweep and nobody marks; the dirty rule reads no more than that
        assert every[4] == (every[2] * len(aj), 0)
        assert dirty[4][0] <= every[4][0] and dirty[4][1] <= dirty[4][0]


def test_every_changing_sweep_raises_the_same_label_entries():
    for ap, aj in _graphs():
        full = sequential(ap, aj)
        inside = [inside_entries(ap, aj, np.arange(len(ap) - 1))]  # the self loops
        for t in range(1, full[2] + 1):
            part = communities(ap, aj, max_sweeps=t)
            _same(part[:2] + (part[3],), sequential(ap, aj, max_sweeps=t)[:2] + (full[3][:t],))
            inside.append(inside_entries(ap, aj, part[0]))
            if full[3][t - 1]:
                assert inside[-1] >= inside[-2] + 2
            else:
                assert inside[-1] == inside[-2]
        assert full[2] <= len(aj) // 2 + 2
        _same(communities(ap, aj, max_sweeps=full[2])[:2], full[:2])


def test_row_order_does_not_matter():
    ap, aj = _random_multigraph(seed=9)
    want = communities(ap, aj)
    rng = np.random.default_rng(1)
    aj = aj.copy()
    for u in range(len(ap) - 1):
        rng.shuffle(aj[ap[u]:ap[u + 1]])
    _same(communities(ap, aj), want)


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


def test_two_cliques_and_a_bridge_by_hand():
    ap, aj = csr(10, np.asarray(_clique(0, 5) + _clique(5, 5) + [(4, 5)], np.int64))
    for run in (sequential, communities):
        label, count, sweeps, changes, _ = run(ap, aj)
        assert label.tolist() == [0] * 5 + [5] * 5 and count == 2 and sweeps == 2 and changes == [8, 0]
    assert len(aj) == 42
    i, s, q = modularity_parts(ap, aj, label)
    assert (i, s) == (40, 882) and q == 40 / 42 - 0.5


def test_star_isolated_vertices_and_self_loops_by_hand():
    for hub in (0, 40):
        ap, aj = csr(41, [(hub, i) for i in range(41) if i != hub])
        label, count, sweeps, changes, _ = communities(ap, aj)
        assert (label == 0).all() and count == 1 and sweeps == 2 and changes == [40, 0]
        _same(sequential(ap, aj), communities(ap, aj))
    # 0, 2 and 5 are isolated, 1 has only a self loop: each keeps its own label
    ap, aj = csr(6, np.asarray([(1, 1), (3, 4)], np.int64))
    label, count, sweeps, _, _ = sequential(ap, aj)
    assert label.tolist() == [0, 1, 2, 3, 3, 5] and count == 5 and sweeps == 2
    # the self loop is stored twice (row 1 has length 2) and 3, 4 share a label: tot = 2 and 2
    assert len(aj) == 4 and modularity_parts(ap, aj, label)[:2] == (4, 2 * 2 + 2 * 2)
    ap, aj = csr(4, np.zeros((0, 2), np.int64))
    _same(sequential(ap, aj), communities(ap, aj))
    assert communities(ap, aj)[0].tolist() == [0, 1, 2, 3] and communities(ap, aj)[1:] == (4, 1, [0], (0, 0))
    assert modularity_parts(ap, aj, np.arange(4)) == (0, 0, 0.0)
    ap, aj = csr(0, np.zeros((0, 2), np.int64))
    _same(sequential(ap, aj), communities(ap, aj))
    assert communities(ap, aj)[1:] == (0, 0, [], (0, 0))


def test_a_repeated_entry_counts_each_time():
    """Two triangles and a vertex between them: it sees each once, so the hash decides; a second
    copy of either edge decides for that side."""
    base = _clique(0, 3) + _clique(4, 3) + [(2, 3), (3, 4)]
    ap, aj = csr(7, np.asarray(base + [(3, 4)], np.int64))
    right = communities(ap, aj)[0]
    _same(sequential(ap, aj), communities(ap, aj))
    ap, aj = csr(7, np.asarray(base + [(2, 3)], np.int64))
    left = communities(ap, aj)[0]
    _same(sequential(ap, aj), communities(ap, aj))
    assert right[3] == right[4] and right[3] != right[2]
    assert left[3] == left[2] and left[3] != left[4]
    plain = communities(*csr(7, np.asarray(base, np.int64)))[0]
    assert plain.tolist() != right.tolist() or plain.tolist() != left.tolist()


def test_modularity_against_networkx():
    nx = pytest.importorskip("networkx")
    for ap, aj in (mtx_csr(CHESAPEAKE), simple_csr(*_random_multigraph())):
        n = len(ap) - 1
        src = np.repeat(np.arange(n), np.diff(ap))
        keep = src != aj
        if not keep.all():  # the formula agrees on graphs without self loops
            ap, aj = csr(n, np.stack([src[keep], aj[keep]], 1), symmetric=False)
            src = np.repeat(np.arange(n), np.diff(ap))
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from((int(a), int(b)) for a, b in zip(src, aj))
        for label in (communities(ap, aj, max_sweeps=1)[0], np.arange(n) % 3, np.zeros(n, np.int64)):
            groups = [set(np.flatnonzero(label == l).tolist()) for l in np.unique(label)]
            assert abs(modularity_parts(ap, aj, label)[2] - nx.community.modularity(G, groups)) < 1e-12


def test_early_stop_is_a_prefix_of_the_full_run():
    ap, aj = _random_multigraph(seed=11)
    full = communities(ap, aj)
    for t in (1, 2):
        part = communities(ap, aj, max_sweeps=t)
        assert part[2] == min(t, full[2]) and part[3] == full[3][:t]
        _same(part, sequential(ap, aj, max_sweeps=t))
