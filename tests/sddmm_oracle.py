"""Oracle of grx_sddmm: the definition in include/essentials_amd.h in numpy float64, and the header's
summation order followed literally in float32.  The checker, never the thing shipped."""
import numpy as np

# the tests build their inputs with these
from hits_oracle import SWEEP_LENGTHS, csr, sweep_ladder, transpose  # noqa: F401

ORDERS = ("tree", "sequential", "lanes_then_sequential")
TILE = 256   # features of a tile
VEC = 4      # features of a lane


def _entries(ap, aj):
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    return np.repeat(np.arange(len(ap) - 1), np.diff(ap)), aj[:ap[-1]]


def sddmm(ap, aj, u, v):
    """out[e] = <u[row(e)], v[col(e)]> in float64, one per entry in the order of the column array."""
    row, col = _entries(ap, aj)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    assert u.ndim == 2 and v.ndim == 2 and u.shape[1] == v.shape[1]
    return (u[row] * v[col]).sum(axis=1)


def _step(acc, a, b):
    """acc = fma(a, b, acc) in float32, for every entry at once."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _add(a, b):
    return (a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def lanes_of(n):
    """The smallest power of two >= ceil(n / 4): the lanes of a tile of n features."""
    quads, L = -(-n // VEC), 1
    while L < quads:
        L *= 2
    return L


def _tile_sum(a, b, order):
    """The sum over one tile's features ([entries, n] each) -> float32 [entries]."""
    n = a.shape[1]
    L = lanes_of(n)
    lanes = []
    for l in range(L):  # lane l: features 4 l .. 4 l + 3 that exist, ascending, from 0.0f
        p = np.zeros(a.shape[0], np.float32)
        for f in range(VEC * l, min(VEC * l + VEC, n)):
            p = _step(p, a[:, f], b[:, f])
        lanes.append(p)
    if order == "lanes_then_sequential":
        acc = lanes[0]
        for p in lanes[1:]:
            acc = _add(acc, p)
        return acc
    d = L // 2
    while d:  # the butterfly: p[l] = p[l] + p[l ^ d], d = L / 2, ..., 1; every lane ends with the same value
        lanes = [_add(lanes[l], lanes[l ^ d]) for l in range(L)]
        d //= 2
    for p in lanes[1:]:
        assert (p.view(np.uint32) == lanes[0].view(np.uint32)).all()
    return lanes[0]


def sddmm_in_order(ap, aj, u, v, order="tree"):
    """The float32 dot products summed as the header of grx_sddmm writes it (order="tree"): features in
    tiles of 256; within a tile of n features L = lanes_of(n) lanes, lane l takes features 4 l .. 4 l + 3
    in ascending order, one fused multiply-add each from 0.0f; the partials meet in the butterfly
    d = L / 2, ..., 1 with plain adds; tile sums are added in ascending tile order.

    A step is float32(float64(acc) + float64(a) * float64(b)).  That EQUALS the fused multiply-add on
    the inputs this function is used with (order_inputs, and small integers), by the argument of
    spmm_oracle.spmm_in_order: every a and b is an integer, a product a * b has at most 24 significant
    bits, and every sum stays far below 2**50, so the float64 product and the float64 sum are exact and
    the one rounding is the conversion to float32.  The same holds for the plain adds.  On general
    floats the equality is not claimed.

    order="sequential" takes all F features in ascending order into one accumulator, and
    order="lanes_then_sequential" forms the lanes' partials as written and adds them lane 0, 1, 2, ...
    instead of in the butterfly: other orders over the same terms, which the tests use to show that
    their inputs tell orders apart.  -> float32 [nnz]"""
    assert order in ORDERS
    row, col = _entries(ap, aj)
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    assert u.ndim == 2 and v.ndim == 2 and u.shape[1] == v.shape[1]
    a, b = u[row], v[col]
    F = u.shape[1]
    if order == "sequential":
        acc = np.zeros(len(row), np.float32)
        for f in range(F):
            acc = _step(acc, a[:, f], b[:, f])
        return acc
    out = np.zeros(len(row), np.float32)
    for f0 in range(0, F, TILE):
        t = _tile_sum(a[:, f0:f0 + TILE], b[:, f0:f0 + TILE], order)
        out = t if f0 == 0 else _add(out, t)
    return out


def order_inputs(rng, shape):
    """Features on which sddmm_in_order is the fused arithmetic AND summation orders differ: odd
    integers in [2**11, 2**12) for both matrices.  A product is odd, in [2**22, 2**24): at most 24
    significant bits; a dot product of F <= 2**20 features stays far below 2**50; and two products
    already sum to more than 24 bits, so nearly every step rounds and the result depends on the order
    from a few features on."""
    return (2 * rng.integers(2 ** 10, 2 ** 11, shape) + 1).astype(np.float32)
