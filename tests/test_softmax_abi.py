"""CPU checks of the edge softmax's place in the product boundary (the header declares grx_edge_softmax and
grx_edge_softmax_backward, the library exports them, the Python layer offers essentials_amd.edge_softmax,
.edge_softmax_backward and .edge_softmax_autograd) and of the oracle the GPU tests compare against
(tests/softmax_oracle.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from softmax_oracle import (ORDERS, backward, backward_in_order, csr, edge_softmax, forward_bound, groups,
                            order_inputs)
from test_sddmm_abi import declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "essentials_amd.h")
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def test_header_declares_the_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for d in ("int grx_edge_softmax(grx_context_t ctx, grx_graph_t g, int32_t by_column, const float* d_scores, "
              "float* d_out, const grx_options* opt, grx_stats* stats)",
              "int grx_edge_softmax_backward(grx_context_t ctx, grx_graph_t g, int32_t by_column, "
              "const float* d_probabilities, const float* d_grad, float* d_out, const grx_options* opt, "
              "grx_stats* stats)"):
        assert re.search(declaration(d), text), d
    assert re.search(r"#define\s+GRX_ABI_VERSION\s+1\b", text)


def test_library_exports_the_calls():
    from essentials_amd.build import build
    lib = C.CDLL(build())
    assert hasattr(lib, "grx_edge_softmax") and hasattr(lib, "grx_edge_softmax_backward")


def test_python_layer_offers_the_calls():
    import essentials_amd as ea
    from essentials_amd.api import _SIGNATURES
    for name in ("edge_softmax", "edge_softmax_backward", "edge_softmax_autograd"):
        assert callable(getattr(ea, name)) and name in ea.__all__
    forward = inspect.signature(ea.edge_softmax).parameters
    assert list(forward) == ["ctx", "g", "scores", "by", "out", "options"]
    back = inspect.signature(ea.edge_softmax_backward).parameters
    assert list(back) == ["ctx", "g", "probabilities", "grad", "by", "out", "options"]
    auto = inspect.signature(ea.edge_softmax_autograd).parameters
    assert list(auto) == ["ctx", "g", "scores", "by"]
    for p in (forward, back, auto):
        assert p["by"].default == "row"
    assert forward["out"].default is None and back["options"].default is None
    assert len(_SIGNATURES["grx_edge_softmax"][1]) == 7 and len(_SIGNATURES["grx_edge_softmax_backward"][1]) == 8


# ---- the oracle gives the hand values ------------------------------------------------------------------

def hand_graph():
    return csr(3, [(0, 1), (0, 3), (2, 0), (2, 0)], symmetric=False)[:2]  # 3 x 4, row 1 empty, a repeat


def test_oracle_by_hand():
    ap, aj = hand_graph()
    assert [g.tolist() for g in groups(ap, aj, "row")] == [[0, 1], [], [2, 3]]
    assert [g.tolist() for g in groups(ap, aj, "column")] == [[2, 3], [0], [], [1]]
    ln = np.log
    out = edge_softmax(ap, aj, [ln(1.0), ln(3.0), ln(2.0), ln(6.0)])
    assert np.allclose(out, [0.25, 0.75, 0.25, 0.75], rtol=1e-15, atol=0)
    out = edge_softmax(ap, aj, [5.0, -7.0, ln(1.0), ln(4.0)], "column")
    assert np.allclose(out, [1.0, 1.0, 0.2, 0.8], rtol=1e-15, atol=0)
    inf, nan = np.inf, np.nan
    assert edge_softmax(ap, aj, [0.0, -inf, -inf, -inf]).tolist() == [1.0, 0.0, 0.0, 0.0]   # masked entry, masked group
    assert np.isnan(edge_softmax(ap, aj, [nan, -inf, 1.0, inf])).all()                      # NaN beside -inf; +inf
    mixed = edge_softmax(ap, aj, [1.0, 1.0, nan, 0.0])
    assert mixed[:2].tolist() == [0.5, 0.5] and np.isnan(mixed[2:]).all()
    # backward: D = 0.25 * 8 + 0.75 * 4 = 5 in row 0, 0.5 * 2 + 0.5 * 6 = 4 in row 2
    a, t = [0.25, 0.75, 0.5, 0.5], [8.0, 4.0, 2.0, 6.0]
    want = [0.75, -0.75, -1.0, 1.0]
    assert backward(ap, aj, a, t).tolist() == want
    for order in ORDERS:
        assert backward_in_order(ap, aj, a, t, 64, "row", order).tolist() == want
    # by column: {2, 3} has D = 4, {0} has D = 2, {1} has D = 3
    assert backward(ap, aj, a, t, "column").tolist() == [0.25 * 6, 0.75 * 1, -1.0, 1.0]
    assert backward_in_order(ap, aj, a, t, 64, "column").tolist() == [1.5, 0.75, -1.0, 1.0]


def _chesapeake():
    """The golden graph as a symmetric CSR, read without the engine (39 vertices, 340 entries)."""
    rows, cols = [], []
    with open(CHESAPEAKE) as f:
        lines = [l for l in f if not l.startswith("%")]
    n = int(lines[0].split()[0])
    for l in lines[1:]:
        r, c = (int(x) - 1 for x in l.split()[:2])
        rows.append((r, c))
    return n, csr(n, rows, symmetric=True)


@pytest.mark.parametrize("by", ["row", "column"])
def test_oracle_is_torch_softmax_per_group(by):
    import torch
    n, (ap, aj, _) = _chesapeake()
    assert len(aj) == 340
    s = np.random.default_rng(5).uniform(-8, 8, len(aj))
    out = edge_softmax(ap, aj, s, by)
    seen = 0
    for at in groups(ap, aj, by):
        if len(at) == 0:
            continue
        want = torch.softmax(torch.from_numpy(s[at]), dim=0).numpy()
        assert np.allclose(out[at], want, rtol=1e-14, atol=0)
        seen += len(at)
    assert seen == len(aj)
    sums = np.array([out[at].sum() for at in groups(ap, aj, by) if len(at)])
    assert np.allclose(sums, 1.0, rtol=1e-14)


# ---- the order inputs tell orders apart, single entries do not -----------------------------------------

def dense_groups(count, n):
    return (np.arange(count + 1) * n).astype(np.int32), np.zeros(count * n, np.int32)


@pytest.mark.parametrize("n", [64, 200, 1030])
def test_order_inputs_tell_orders_apart(n):
    rng = np.random.default_rng(17)
    ap, aj = dense_groups(24, n)
    a, t = order_inputs(rng, 24 * n)
    assert ((a * 256) == np.round(a * 256)).all() and a.min() >= 0 and a.max() <= 1
    assert (t % 2 == 1).all() and t.min() >= 2 ** 14 and t.max() < 2 ** 15
    for segment in (64, 512):
        lanes = backward_in_order(ap, aj, a, t, segment)
        for other in ("sequential", "reversed"):
            out = backward_in_order(ap, aj, a, t, segment, "row", other)
            differs = np.mean([(out[g].view(np.uint32) != lanes[g].view(np.uint32)).any() for g in groups(ap, aj)])
            assert differs > 0.25, (other, segment, differs)
        # every order is a float32 evaluation of the same expression: near the float64 value
        exact = backward(ap, aj, a, t)
        scale = np.abs(a.astype(np.float64) * t).reshape(24, n).sum(axis=1).repeat(n)
        assert (np.abs(lanes - exact) <= 1.01 * (n + 3) * 2.0 ** -24 * (scale + np.abs(t))).all()


def test_the_orders_coincide_on_single_entries():
    rng = np.random.default_rng(19)
    ap, aj = dense_groups(50, 1)
    a, t = order_inputs(rng, 50)
    lanes = backward_in_order(ap, aj, a, t, 64)
    for other in ("sequential", "reversed"):
        assert (backward_in_order(ap, aj, a, t, 64, "row", other).view(np.uint32) == lanes.view(np.uint32)).all()
    d = (a.astype(np.float64) * t).astype(np.float32)  # the one product, rounded; then the two rounded steps
    want = (a.astype(np.float64) * (t.astype(np.float64) - d).astype(np.float32)).astype(np.float32)
    assert (lanes.view(np.uint32) == want.view(np.uint32)).all()


def test_small_integers_are_exact_in_every_order():
    rng = np.random.default_rng(18)
    ap, aj = dense_groups(6, 300)
    a = rng.integers(0, 4, 1800).astype(np.float32)
    t = rng.integers(-8, 9, 1800).astype(np.float32)
    want = backward(ap, aj, a, t)
    assert (np.abs(want) < 2 ** 24).all()
    for order in ORDERS:
        for segment in (64, 512):
            assert (backward_in_order(ap, aj, a, t, segment, "row", order).astype(np.float64) == want).all()


def test_the_forward_bound():
    assert forward_bound(1, 0, 0) == 1.01 * 2.0 ** -24
    assert forward_bound(100, 32, 2) == 1.01 * (2 * 36 + 100) * 2.0 ** -24
    assert forward_bound(16, 32) == forward_bound(16, 32, 2)
