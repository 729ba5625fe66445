"""Oracle of grx_spmm: the definition in include/essentials_amd.h in numpy float64, and the header's
summation order followed literally in float32.  The checker, never the thing shipped."""
import numpy as np

# the tests build their inputs with these
from hits_oracle import SWEEP_LENGTHS, csr, sweep_ladder, transpose  # noqa: F401

ORDERS = ("row", "reversed", "lanes16")


def _rows(ap, aj, aw):
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    aw = np.asarray(aw, np.float32).astype(np.float64)
    return np.repeat(np.arange(len(ap) - 1), np.diff(ap)), aj, aw


def spmm(ap, aj, aw, x, n_cols=None, transpose=False):
    """Y = A X (float64, [n_rows, F]), or Y = A^T X: Y[c, f] = sum over entries (r -> c, w) of
    X[r, f] * w, [n_cols, F]."""
    row, col, w = _rows(ap, aj, aw)
    n = len(ap) - 1
    x = np.asarray(x, np.float64)
    assert x.ndim == 2
    m = (n if n_cols is None else n_cols) if transpose else n
    y = np.zeros((m, x.shape[1]))
    if transpose:
        np.add.at(y, col, x[row] * w[:, None])
    else:
        np.add.at(y, row, x[col] * w[:, None])
    return y


def _step(acc, x, w):
    """acc = fma(x, w, acc) in float32, for every feature of one entry."""
    return (acc.astype(np.float64) + x.astype(np.float64) * np.float64(w)).astype(np.float32)


def _add(a, b):
    return (a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def _segment_sum(x, cols, weights, order):
    F = x.shape[1]
    if order == "lanes16":  # grx_spmv's: lane l takes entries l, l + 16, ..., then the butterfly 8, 4, 2, 1
        lanes = []
        for l in range(16):
            acc = np.zeros(F, np.float32)
            for c, w in zip(cols[l::16], weights[l::16]):
                acc = _step(acc, x[c], w)
            lanes.append(acc)
        for d in (8, 4, 2, 1):
            lanes = [_add(lanes[l], lanes[l ^ d]) for l in range(16)]
        return lanes[0]
    if order == "reversed":
        cols, weights = cols[::-1], weights[::-1]
    acc = np.zeros(F, np.float32)
    for c, w in zip(cols, weights):
        acc = _step(acc, x[c], w)
    return acc


def spmm_in_order(ap, aj, aw, x, segment, order="row"):
    """The float32 product summed as the header of grx_spmm writes it (order="row"): per output element
    the row's entries in segments of `segment` consecutive entries; a segment's sum starts from 0.0f and
    takes its entries in row order, one fused multiply-add each; a row of at most `segment` entries
    delivers that sum, a longer one ((p0 + p1) + p2) + ... in segment order.

    A step is float32(float64(acc) + float64(x) * float64(w)).  That EQUALS the fused multiply-add on
    the inputs this function is used with: every x and every w is an integer, every product x * w has
    at most 24 significant bits, and every row total is below 2**50.  The float64 product is then exact
    (24 bits fit 53), acc is an integer below 2**50 and so is the sum of the two, which float64 holds
    exactly; the one rounding is the conversion to float32 -- the rounding a fused multiply-add performs
    on the exact x * w + acc.  The same holds for the plain adds of the partial sums.  On general floats
    the float64 sum may round first and the equality is not claimed.

    order="reversed" takes each segment's entries last to first and order="lanes16" sums a segment the
    way grx_spmv does (16 interleaved lanes and a butterfly): other orders over the same segments,
    which the tests use to show that their inputs tell orders apart.  -> float32 [n_rows, F]"""
    assert order in ORDERS and segment >= 1
    ap = np.asarray(ap, np.int64)
    aj = np.asarray(aj, np.int64)
    aw = np.asarray(aw, np.float32)
    x = np.asarray(x, np.float32)
    assert x.ndim == 2
    y = np.zeros((len(ap) - 1, x.shape[1]), np.float32)
    for r in range(len(ap) - 1):
        lo, hi = ap[r], ap[r + 1]
        partial = [_segment_sum(x, aj[s:min(s + segment, hi)], aw[s:min(s + segment, hi)], order)
                   for s in range(lo, hi, segment)]
        if partial:
            acc = partial[0]
            for p in partial[1:]:
                acc = _add(acc, p)
            y[r] = acc
    return y


def order_inputs(rng, shape):
    """Features on which spmm_in_order is the fused arithmetic AND summation orders differ: odd integers
    in [2**17, 2**18).  With the project's integer weights 1..64 (at most 6 bits) a product has at most
    24 significant bits and is below 2**24, so a row of up to 2**20 entries stays far below 2**50; two
    products already sum to more than 24 bits, so nearly every step rounds and the result depends on
    the order from the first few entries of a segment on."""
    return (2 * rng.integers(2 ** 16, 2 ** 17, shape) + 1).astype(np.float32)
