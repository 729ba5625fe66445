"""Oracle of grx_edge_softmax and grx_edge_softmax_backward: the definitions in include/essentials_amd.h in
numpy float64, the header's summation order of the backward pass followed literally in float32, and the
error bound of the forward pass.  The checker, never the thing shipped."""
import numpy as np

# the tests build their inputs with these
from hits_oracle import SWEEP_LENGTHS, csr, sweep_ladder, transpose  # noqa: F401

ORDERS = ("lanes16", "sequential", "reversed")
BYS = ("row", "column")
ULP = 2.0 ** -24
EXPF_ULP = 2  # see forward_bound


def groups(ap, aj, by="row"):
    """The groups as arrays of positions in the CSR's column array, each in group order: the entries of
    a row as they lie, or those of a column in ascending position (a stable sort by column, which is
    what the in-rows are).  One array per row, or per column up to the largest one present."""
    assert by in BYS
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    if by == "row":
        return [np.arange(ap[r], ap[r + 1]) for r in range(len(ap) - 1)]
    aj = aj[:ap[-1]]
    order = np.argsort(aj, kind="stable")
    cuts = np.cumsum(np.bincount(aj, minlength=1))[:-1] if len(aj) else []
    return np.split(order, cuts)


def edge_softmax(ap, aj, s, by="row"):
    """out[e] = exp(s[e] - m) / sum over e's group of exp(s[e'] - m) in float64.  A group that holds a
    NaN or a +inf is NaN throughout (what torch.softmax gives: inf - inf), one whose scores are all
    -inf is 0 throughout (the header's rule; torch gives NaN there)."""
    s = np.asarray(s, np.float64)
    out = np.zeros(len(s))
    for at in groups(ap, aj, by):
        if len(at) == 0:
            continue
        x = s[at]
        if np.isnan(x).any() or (x == np.inf).any():
            out[at] = np.nan
        elif (x == -np.inf).all():
            out[at] = 0.0
        else:
            p = np.exp(x - x.max())
            out[at] = p / p.sum()
    return out


def backward(ap, aj, a, t, by="row"):
    """out[e] = a[e] * (t[e] - sum over e's group of a[e'] * t[e']) in float64."""
    a, t = np.asarray(a, np.float64), np.asarray(t, np.float64)
    out = np.zeros(len(a))
    for at in groups(ap, aj, by):
        out[at] = a[at] * (t[at] - (a[at] * t[at]).sum())
    return out


def _f32(x):
    """One rounding: the float64 value as the nearest float32, kept as a Python float."""
    return float(np.float32(x))


def _segment_dot(a, t, order):
    if order == "lanes16":  # lane l takes entries l, l + 16, ..., then the butterfly 8, 4, 2, 1
        lanes = []
        for l in range(16):
            acc = 0.0
            for x, y in zip(a[l::16], t[l::16]):
                acc = _f32(acc + x * y)
            lanes.append(acc)
        for d in (8, 4, 2, 1):
            lanes = [_f32(lanes[l] + lanes[l ^ d]) for l in range(16)]
        assert len(set(lanes)) == 1
        return lanes[0]
    if order == "reversed":
        a, t = a[::-1], t[::-1]
    acc = 0.0
    for x, y in zip(a, t):
        acc = _f32(acc + x * y)
    return acc


def backward_in_order(ap, aj, a, t, segment, by="row", order="lanes16"):
    """The float32 backward pass as the header of grx_edge_softmax_backward writes it (order="lanes16"):
    per group D over segments of `segment` consecutive entries; within a segment lane l of 16 takes
    entries l, l + 16, ... in order, acc = fma(a[e], t[e], acc) from 0.0f; the 16 lane sums meet in the
    butterfly 8, 4, 2, 1; a group of at most `segment` entries has that sum for D, a longer one
    ((0.0f + D0) + D1) + ... in segment order; out[e] = a[e] * (t[e] - D), a rounded subtraction and a
    rounded multiplication.

    Every step is computed as float32(float64 operation).  That EQUALS the float32 arithmetic (fused
    where it is fused) on the inputs this function is used with -- order_inputs, and small integers --
    by the argument in order_inputs' docstring; on general floats the equality is not claimed.

    order="sequential" takes a segment's entries first to last into one accumulator and
    order="reversed" last to first: other orders over the same segments, which the tests use to show
    that their inputs tell orders apart.  -> float32 [nnz]"""
    assert order in ORDERS and segment >= 1
    a32, t32 = np.asarray(a, np.float32), np.asarray(t, np.float32)
    a, t = a32.astype(np.float64), t32.astype(np.float64)
    out = np.zeros(len(a), np.float32)
    for at in groups(ap, aj, by):
        n = len(at)
        if n == 0:
            continue
        x, y = a[at].tolist(), t[at].tolist()
        partial = [_segment_dot(x[lo:lo + segment], y[lo:lo + segment], order) for lo in range(0, n, segment)]
        dot = partial[0]
        if len(partial) > 1:
            dot = 0.0
            for p in partial:
                dot = _f32(dot + p)
        out[at] = [np.float32(xe * _f32(ye - dot)) for xe, ye in zip(x, y)]
    return out


def order_inputs(rng, n):
    """(a, t) on which backward_in_order is the device's float32 arithmetic AND summation orders differ:
    a = k / 256 with k an integer in 0..256, t an odd integer in [2**14, 2**15).

    Why the float64 steps equal the (fused) float32 ones: a product a * t = k * t / 256 has at most
    9 + 15 = 24 significant bits and is a multiple of 2**-8, so the float64 product is exact.  Every
    accumulator is a float32 that was rounded from a multiple of 2**-8, hence itself one, and every
    total stays below 2**15 * 2**30 = 2**45 for any group this project can hold; a multiple of 2**-8
    below 2**45 has at most 53 bits, so acc + a * t is exact in float64 and the conversion to float32
    is its only rounding -- the one rounding a fused multiply-add performs on the exact a * t + acc.
    The same holds for the plain adds of lane sums and segment sums.  t - D is an integer minus a
    multiple of 2**-8, both below 2**45: exact in float64, then rounded once as the device's
    subtraction rounds.  a * (t - D) is 9 bits times a float32's 24: 33 bits, exact in float64, then
    rounded once as the device's multiplication rounds.
    Why orders differ: a lane's second product already carries the sum past 24 bits (15 bits above
    the binary point, 8 below, then a carry), so nearly every step rounds from then on."""
    a = (rng.integers(0, 257, n) / 256.0).astype(np.float32)
    t = (2 * rng.integers(2 ** 13, 2 ** 14, n) + 1).astype(np.float32)
    return a, t


def forward_bound(n, spread, E=EXPF_ULP):
    """Bounds |out[e] - exact| / exact of grx_edge_softmax against float64 for a group of n entries
    whose scores lie within `spread` of their maximum (max(m - s) <= spread, all finite), u = 2**-24:

      the subtraction s - m rounds once: an absolute error of at most spread * u in the argument of
        exp, which is a relative error of (about) spread * u in p;
      expf is within E ulp, and an ulp is at most 2 u relative: 2 E u;
      so every p[e] carries at most (spread + 2 E) u -- the numerator does, and so does the
        denominator, a sum of non-negative terms each within that, where nothing cancels;
      the sum adds at most n - 1 roundings on any path from a term to the total, in any order: (n - 1) u;
      the division rounds once: u.

    Together 2 (spread + 2 E) u + (n - 1) u + u, and 1 % on top for the second-order terms:
    1.01 * (2 * (spread + 2 * E) + n) * 2**-24.

    E: no copy of HIP's math API accuracy table is at hand where this was written, so E = 2 is an
    ASSUMPTION (the tables of such libraries give 1 or 2 ulp for expf); tools/softmax_probe.py records
    how much of the bound the device uses."""
    return 1.01 * (2.0 * (spread + 2.0 * E) + n) * ULP
