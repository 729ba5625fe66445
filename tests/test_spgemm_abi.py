"""CPU checks of the sparse matrix product's place in the product boundary (the header declares
grx_spgemm, the library exports it, the Python layer offers essentials_amd.spgemm) and of the oracle
the GPU tests compare against (tests/spgemm_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spgemm_oracle import KNOWN, csr, product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def test_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_spgemm\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+a,\s*grx_graph_t\s+b,"
                     r"\s*grx_graph_t\s*\*\s*out,", text)


def test_library_exports():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_spgemm")


def test_python_layer_offers_spgemm():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.spgemm) and "spgemm" in ea.__all__
    assert "grx_spgemm" in _SIGNATURES


def test_oracle_known_answer():
    a, b = csr(*KNOWN["A"]), csr(*KNOWN["B"])
    cp, cj, cx64, terms, abs_sum, products = product(*a, *b, 3)
    want_p, want_j, want_x = KNOWN["C"]
    assert cp.dtype == np.int32 and cj.dtype == np.int32
    assert cp.tolist() == want_p and cj.tolist() == want_j and cx64.tolist() == want_x
    assert terms.tolist() == [2, 1, 1, 1] and abs_sum.tolist() == want_x and products == 5


def _random_pair(seed=3):
    """200x150 . 150x120 with repeated entries and, in row 0, a +1 / -1 pair that cancels."""
    rng = np.random.default_rng(seed)
    ea_ = [(int(r), int(c), float(v)) for r, c, v in zip(rng.integers(1, 200, 1500), rng.integers(0, 149, 1500),
                                                        rng.choice([-3, -2, -1, 1, 2, 3], 1500))]
    eb = [(int(r), int(c), float(v)) for r, c, v in zip(rng.integers(0, 149, 1200), rng.integers(0, 120, 1200),
                                                        rng.choice([-3, -2, -1, 1, 2, 3], 1200))]
    ea_ += ea_[:100]  # repeats
    eb += eb[:100]
    # row 0 of A meets only row 149 of B, twice, with opposite signs: C[0, 7] = 1 * 1 + (-1) * 1 = 0
    ea_ += [(0, 149, 1.0), (0, 149, -1.0)]
    eb += [(149, 7, 1.0)]
    return csr(200, 150, ea_), csr(150, 120, eb)


def test_oracle_matches_scipy():
    sp = pytest.importorskip("scipy.sparse")
    (ap, aj, ax), (bp, bj, bx) = _random_pair()
    cp, cj, cx64, terms, abs_sum, products = product(ap, aj, ax, bp, bj, bx, 120)
    A = sp.csr_matrix((ax.astype(np.float64), aj, ap), shape=(200, 150))
    B = sp.csr_matrix((bx.astype(np.float64), bj, bp), shape=(150, 120))
    S = (A @ B).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    # scipy prunes entries that sum to zero: compare the values as dense, and take the structural
    # pattern from the product of the magnitudes, where nothing cancels
    dense = np.zeros((200, 120))
    rows = np.repeat(np.arange(200), np.diff(cp))
    dense[rows, cj] = cx64
    assert (dense == S.toarray()).all()
    P = (sp.csr_matrix((np.abs(ax).astype(np.float64), aj, ap), shape=(200, 150)) @
         sp.csr_matrix((np.abs(bx).astype(np.float64), bj, bp), shape=(150, 120))).tocsr()
    P.sum_duplicates()
    P.sort_indices()
    assert P.indptr.tolist() == cp.tolist() and P.indices.tolist() == cj.tolist()
    assert (P.data == abs_sum).all() and S.nnz < P.nnz
    at = cp[0] + int(np.searchsorted(cj[cp[0]:cp[1]], 7))
    assert cj[at] == 7 and cx64[at] == 0.0 and terms[at] == 2 and abs_sum[at] == 2.0
    assert products == int(terms.sum())


def test_oracle_ignores_the_order_within_a_row():
    (ap, aj, ax), (bp, bj, bx) = _random_pair()
    want = product(ap, aj, ax, bp, bj, bx, 120)
    rng = np.random.default_rng(1)

    def shuffled(p, j, x):
        j, x = j.copy(), x.copy()
        for u in range(len(p) - 1):
            perm = rng.permutation(p[u + 1] - p[u]) + p[u]
            j[p[u]:p[u + 1]], x[p[u]:p[u + 1]] = j[perm], x[perm]
        return p, j, x
    got = product(*shuffled(ap, aj, ax), *shuffled(bp, bj, bx), 120)
    for w, g in zip(want[:5], got[:5]):
        assert (w == g).all()
    assert want[5] == got[5]


def test_oracle_chunks_agree():
    (ap, aj, ax), (bp, bj, bx) = _random_pair()
    want = product(ap, aj, ax, bp, bj, bx, 120)
    got = product(ap, aj, ax, bp, bj, bx, 120, chunk=97)  # rows of A straddle chunks
    for w, g in zip(want[:5], got[:5]):
        assert (w == g).all()


def test_oracle_empty_shapes():
    z = np.zeros(1, np.int32)
    e = np.zeros(0, np.int32)
    cp, cj, cx64, terms, abs_sum, products = product(z, e, e, z, e, e, 0)
    assert cp.tolist() == [0] and len(cj) == 0 and products == 0
    cp, cj, *_ = product(np.zeros(4, np.int32), e, e, np.zeros(6, np.int32), e, e, 2)
    assert cp.tolist() == [0, 0, 0, 0] and len(cj) == 0
