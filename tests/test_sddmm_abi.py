"""CPU checks of the edge-wise products' place in the product boundary (the header declares grx_sddmm and
grx_spmm_values, the library exports them, the Python layer offers essentials_amd.sddmm,
.sddmm_autograd and the `values` keyword of .spmm and .spmm_autograd) and of the oracle the GPU tests
compare against (tests/sddmm_oracle.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sddmm_oracle import csr, lanes_of, order_inputs, sddmm, sddmm_in_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")


def declaration(text):
    """A C declaration as a regular expression that does not mind white space."""
    tokens = re.findall(r"\w+|[^\w\s]", text)
    return r"\b" + r"\s*".join(re.escape(t) for t in tokens) + r"\s*;"


def test_header_declares_the_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for d in ("int grx_sddmm(grx_context_t ctx, grx_graph_t g, int32_t n_features, const float* d_u, int64_t ldu, "
              "const float* d_v, int64_t ldv, float* d_out, const grx_options* opt, grx_stats* stats)",
              "int grx_spmm_values(grx_context_t ctx, grx_graph_t g, const float* d_values, int32_t transpose, "
              "int32_t n_features, const float* d_x, int64_t ldx, float* d_y, int64_t ldy, const grx_options* opt, "
              "grx_stats* stats)"):
        assert re.search(declaration(d), text), d
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", text)


def test_library_exports_the_calls():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_sddmm") and hasattr(lib, "grx_spmm_values")


def test_python_layer_offers_the_calls():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    assert callable(ea.sddmm) and callable(ea.sddmm_autograd)
    assert "sddmm" in ea.__all__ and "sddmm_autograd" in ea.__all__
    assert list(inspect.signature(ea.sddmm).parameters) == ["ctx", "g", "u", "v", "out", "options"]
    assert list(inspect.signature(ea.sddmm_autograd).parameters) == ["ctx", "g", "u", "v"]
    spmm = inspect.signature(ea.spmm).parameters
    assert list(spmm)[-1] == "values" and spmm["values"].default is None
    assert list(spmm)[:6] == ["ctx", "g", "x", "transpose", "y", "options"]  # what callers pass by position
    auto = inspect.signature(ea.spmm_autograd).parameters
    assert list(auto) == ["ctx", "g", "x", "values"] and auto["values"].default is None
    assert len(_SIGNATURES["grx_sddmm"][1]) == 10 and len(_SIGNATURES["grx_spmm_values"][1]) == 11
    assert len(_SIGNATURES["grx_spmm"][1]) == 10


# ---- the oracle gives the hand values ------------------------------------------------------------------

def test_oracle_by_hand():
    ap, aj, _ = csr(3, [(0, 1), (0, 3), (2, 0), (2, 0)], symmetric=False)  # 3 x 4, row 1 empty, a repeat
    u = np.array([[1.0, 2.0, 3.0], [9.0, 9.0, 9.0], [-1.0, 0.5, 4.0]])
    v = np.array([[2.0, 4.0, 1.0], [1.0, 1.0, 1.0], [7.0, 7.0, 7.0], [0.0, -1.0, 10.0]])
    want = [6.0, 28.0, 4.0, 4.0]  # <u0, v1>, <u0, v3>, <u2, v0> twice
    assert sddmm(ap, aj, u, v).tolist() == want
    for order in ("tree", "sequential", "lanes_then_sequential"):
        assert sddmm_in_order(ap, aj, u, v, order).tolist() == want


def test_the_lanes_of_a_tile():
    assert [lanes_of(n) for n in (1, 4, 5, 8, 9, 16, 17, 37, 64, 65, 128, 129, 256)] == \
        [1, 1, 2, 2, 4, 4, 8, 16, 16, 32, 32, 64, 64]


# ---- the order inputs tell orders apart, the exact inputs do not ---------------------------------------

def dense_rows(rng, rows=8, columns=64):
    """Every row meets every column once: rows * columns entries."""
    ap = (np.arange(rows + 1) * columns).astype(np.int32)
    aj = np.concatenate([rng.permutation(columns) for _ in range(rows)]).astype(np.int32)
    return ap, aj


@pytest.mark.parametrize("F", [37, 260])
def test_order_inputs_tell_orders_apart(F):
    rng = np.random.default_rng(17)
    ap, aj = dense_rows(rng)
    u, v = order_inputs(rng, (8, F)), order_inputs(rng, (64, F))
    for x in (u, v):
        assert (x == np.round(x)).all() and (x % 2 == 1).all() and x.min() >= 2 ** 11 and x.max() < 2 ** 12
    total = sddmm(ap, aj, u, v)
    assert total.max() < 2.0 ** 50 and u.max() * v.max() < 2.0 ** 24  # what sddmm_in_order's equality needs
    tree = sddmm_in_order(ap, aj, u, v, "tree")
    for other in ("sequential", "lanes_then_sequential"):
        out = sddmm_in_order(ap, aj, u, v, other)
        differs = (out.view(np.uint32) != tree.view(np.uint32)).mean()
        assert differs > 0.25, (other, differs)
    # every order is a float32 summation of the same terms: within the bound any order obeys
    bound = 1.01 * (F + 1) * 2.0 ** -24 * total
    assert (np.abs(tree.astype(np.float64) - total) <= bound).all()


def test_the_orders_coincide_on_a_lane_or_two():
    """Up to F = 5 there is nothing to reorder: one lane, or one lane and a single term."""
    rng = np.random.default_rng(19)
    ap, aj = dense_rows(rng)
    for F in (1, 4, 5):
        u, v = order_inputs(rng, (8, F)), order_inputs(rng, (64, F))
        tree = sddmm_in_order(ap, aj, u, v, "tree")
        for other in ("sequential", "lanes_then_sequential"):
            assert (sddmm_in_order(ap, aj, u, v, other).view(np.uint32) == tree.view(np.uint32)).all()


@pytest.mark.parametrize("F", [37, 260])
def test_small_integers_are_exact_in_every_order(F):
    rng = np.random.default_rng(18)
    ap, aj = dense_rows(rng)
    u = rng.integers(0, 16, (8, F)).astype(np.float32)
    v = rng.integers(0, 16, (64, F)).astype(np.float32)
    want = sddmm(ap, aj, u, v)
    assert (np.abs(want) < 2 ** 24).all()
    for order in ("tree", "sequential", "lanes_then_sequential"):
        assert (sddmm_in_order(ap, aj, u, v, order).astype(np.float64) == want).all()
