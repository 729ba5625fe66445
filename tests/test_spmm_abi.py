"""CPU checks of the sparse-dense product's place in the product boundary (the header declares grx_spmm,
the library exports it, the Python layer offers essentials_amd.spmm and .spmm_autograd) and of the
oracle the GPU tests compare against (tests/spmm_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hits_oracle import spmv
from spmm_oracle import csr, order_inputs, spmm, spmm_in_order, sweep_ladder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def test_header_declares_the_call():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+grx_spmm\s*\(\s*grx_context_t\s+ctx,\s*grx_graph_t\s+g,\s*int32_t\s+transpose,"
                     r"\s*int32_t\s+n_features,\s*const\s+float\s*\*\s*d_x,\s*int64_t\s+ldx,\s*float\s*\*\s*d_y,"
                     r"\s*int64_t\s+ldy,\s*const\s+grx_options\s*\*\s*opt,\s*grx_stats\s*\*\s*stats\s*\)", text)
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", text)


def test_library_exports_the_call():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_spmm")


def test_python_layer_offers_spmm():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.spmm) and callable(ea.spmm_autograd)
    assert "spmm" in ea.__all__ and "spmm_autograd" in ea.__all__
    assert "grx_spmm" in _SIGNATURES and len(_SIGNATURES["grx_spmm"][1]) == 10


# ---- the oracle gives the hand values ------------------------------------------------------------------

def hand_case():
    ap, aj, aw = csr(3, [(0, 1), (0, 3), (2, 0)], weights=[2, 3, 5], symmetric=False)  # 3 x 4
    return ap, aj, aw


def test_oracle_forward_by_hand():
    ap, aj, aw = hand_case()
    x = np.array([[1.0, -1.0], [10.0, 0.5], [100.0, 7.0], [1000.0, 2.0]])
    assert spmm(ap, aj, aw, x).tolist() == [[3020.0, 7.0], [0.0, 0.0], [5.0, -5.0]]
    for order in ("row", "reversed", "lanes16"):
        assert spmm_in_order(ap, aj, aw, x, 64, order).tolist() == [[3020.0, 7.0], [0.0, 0.0], [5.0, -5.0]]


def test_oracle_transposed_by_hand():
    ap, aj, aw = hand_case()
    x = np.array([[1.0, -1.0], [10.0, 0.5], [100.0, 7.0]])
    assert spmm(ap, aj, aw, x, n_cols=4, transpose=True).tolist() == [[500.0, 35.0], [2.0, -2.0], [0.0, 0.0],
                                                                      [3.0, -3.0]]


def test_one_feature_is_the_vector_product():
    ap, aj, aw = sweep_ladder()
    x = np.random.default_rng(2).standard_normal(37)
    assert (spmm(ap, aj, aw, x[:, None])[:, 0] == spmv(ap, aj, aw, x)).all()
    assert (spmm(ap, aj, aw, x[:, None], transpose=True)[:, 0] == spmv(ap, aj, aw, x, transpose=True)).all()


# ---- the order inputs tell orders apart, the exact inputs do not ---------------------------------------

LENGTHS = [65, 200, 513, 1025]
COLUMNS = 2048


def long_rows(rng, lengths=LENGTHS):
    ap = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    aj = np.concatenate([rng.choice(COLUMNS, d, replace=False) for d in lengths]).astype(np.int32)
    aw = rng.integers(1, 65, len(aj)).astype(np.float32)
    return ap, aj, aw


@pytest.mark.parametrize("segment", [64, 512])
def test_order_inputs_tell_orders_apart(segment):
    rng = np.random.default_rng(17)
    ap, aj, aw = long_rows(rng)
    x = order_inputs(rng, (COLUMNS, 8))
    assert (x == np.round(x)).all() and (x % 2 == 1).all() and x.max() < 2 ** 18
    total = spmm(ap, aj, np.abs(aw), np.abs(x))
    assert total.max() < 2.0 ** 50 and (x.max() * aw.max()) < 2.0 ** 24  # what spmm_in_order's equality needs
    row = spmm_in_order(ap, aj, aw, x, segment, "row")
    for other in ("reversed", "lanes16"):
        y = spmm_in_order(ap, aj, aw, x, segment, other)
        differs = (y.view(np.uint32) != row.view(np.uint32)).any(axis=1)
        assert differs.all(), (other, dict(zip(LENGTHS, differs.tolist())))
    # every order is a float32 summation of the same terms: within the bound any order obeys
    bound = 1.01 * (np.diff(ap)[:, None] + 1) * 2.0 ** -24 * total
    assert (np.abs(row.astype(np.float64) - spmm(ap, aj, aw, x)) <= bound).all()


@pytest.mark.parametrize("segment", [64, 512])
def test_small_integers_are_exact_in_every_order(segment):
    rng = np.random.default_rng(18)
    ap, aj, aw = long_rows(rng)
    x = rng.integers(0, 16, (COLUMNS, 2)).astype(np.float32)
    want = spmm(ap, aj, aw, x)
    assert (np.abs(want) < 2 ** 24).all()
    for order in ("row", "reversed", "lanes16"):
        assert (spmm_in_order(ap, aj, aw, x, segment, order).astype(np.float64) == want).all()
