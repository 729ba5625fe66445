"""The sparse matrix product C = A * B of two CSR matrices in plain numpy (the GPU machine may lack
scipy): every product A[i,k] * B[k,j] is expanded, in chunks of a few million, under the key
i * n_cols + j; the distinct keys are C's pattern -- sorted, so rows come out by ascending column --
and per key the float64 sum, the number of products and the sum of their magnitudes are gathered.
An entry whose products cancel stays: the pattern is structural."""
import numpy as np


def product(ap, aj, ax, bp, bj, bx, n_cols, chunk=1 << 22):
    """(cp int32, cj int32, cx64 float64, terms int64, abs_sum float64, products int)."""
    ap, bp = np.asarray(ap, np.int64), np.asarray(bp, np.int64)
    n = len(ap) - 1
    na = int(ap[-1]) if n else 0
    aj = np.asarray(aj, np.int64)[:na]
    ax = np.asarray(ax, np.float64)[:na]
    bj = np.asarray(bj, np.int64)
    bx = np.asarray(bx, np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    lens = (bp[aj + 1] - bp[aj]) if na else np.zeros(0, np.int64)
    work = np.cumsum(lens)
    products = int(work[-1]) if na else 0
    keys, sums, terms, mags = [], [], [], []
    lo = 0
    while lo < na:
        hi = int(np.searchsorted(work, (work[lo - 1] if lo else 0) + chunk, side="right"))
        hi = max(hi, lo + 1)
        l = lens[lo:hi]
        m = int(l.sum())
        if m:
            first = np.cumsum(l) - l
            pos = np.repeat(bp[aj[lo:hi]] - first, l) + np.arange(m)
            key = np.repeat(rows[lo:hi], l) * n_cols + bj[pos]
            val = np.repeat(ax[lo:hi], l) * bx[pos]
            uniq, inv = np.unique(key, return_inverse=True)
            keys.append(uniq)
            sums.append(np.bincount(inv, weights=val, minlength=len(uniq)))
            terms.append(np.bincount(inv, minlength=len(uniq)).astype(np.int64))
            mags.append(np.bincount(inv, weights=np.abs(val), minlength=len(uniq)))
        lo = hi
    if keys:
        # a row of A may straddle two chunks: merge the chunks' keys once more
        key = np.concatenate(keys)
        uniq, inv = np.unique(key, return_inverse=True)
        cx64 = np.bincount(inv, weights=np.concatenate(sums), minlength=len(uniq))
        t = np.bincount(inv, weights=np.concatenate(terms), minlength=len(uniq)).astype(np.int64)
        abs_sum = np.bincount(inv, weights=np.concatenate(mags), minlength=len(uniq))
    else:
        uniq = np.zeros(0, np.int64)
        cx64, t, abs_sum = np.zeros(0), np.zeros(0, np.int64), np.zeros(0)
    cp = np.zeros(n + 1, np.int64)
    if len(uniq):
        cp[1:] = np.cumsum(np.bincount(uniq // n_cols, minlength=n))
    cj = (uniq % n_cols) if len(uniq) else uniq
    return cp.astype(np.int32), cj.astype(np.int32), cx64, t, abs_sum, products


def csr(n_rows, n_cols, entries):
    """CSR (int32 offsets, int32 columns, float32 values) of (row, column, value) triples IN THE ORDER
    GIVEN within a row (stable by row): repeats stay repeats."""
    e = np.asarray(entries, np.float64).reshape(-1, 3)
    r = e[:, 0].astype(np.int64)
    order = np.argsort(r, kind="stable")
    ap = np.zeros(n_rows + 1, np.int64)
    ap[1:] = np.cumsum(np.bincount(r, minlength=n_rows))
    return ap.astype(np.int32), e[order, 1].astype(np.int32), e[order, 2].astype(np.float32)


# the pair of the reference's datasets/spgemm (a.mtx, b.mtx) and their product, typed in as data
KNOWN = {
    "A": (3, 3, [(0, 1, 1.0), (0, 2, 1.0), (1, 2, 1.0)]),
    "B": (3, 3, [(1, 0, 1.0), (2, 0, 1.0), (2, 1, 1.0)]),
    "C": ([0, 2, 4, 4], [0, 1, 0, 1], [2.0, 1.0, 1.0, 1.0]),
}
