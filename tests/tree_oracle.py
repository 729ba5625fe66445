"""Oracle of grx_bfs_predecessors and grx_sssp_predecessors: the definition in include/essentials_amd.h
followed literally in numpy.  The checker, never the thing shipped."""
import numpy as np

# the tests build their inputs with these
from ppr_oracle import SWEEP_LENGTHS, csr, sweep_ladder, transpose  # noqa: F401

INT_UNREACHED = 2 ** 31 - 1
FLT_UNREACHED = np.finfo(np.float32).max
NONE = 2 ** 31 - 1


def entries(ap, aj, aw, labels):
    """(u, v, qualifies, violates) per row entry, as the definition tests it."""
    ap, v = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    u = np.repeat(np.arange(len(ap) - 1), np.diff(ap))
    labels = np.asarray(labels)
    if labels.dtype.kind == "i":
        lab = labels.astype(np.int64)
        live = lab[u] != INT_UNREACHED
        c = lab[u] + 1
        qualifies = c == lab[v]
    else:
        assert labels.dtype == np.float32
        live = labels[u] != FLT_UNREACHED
        with np.errstate(over="ignore", invalid="ignore"):
            c = labels[u] + np.asarray(aw, np.float32)  # one float32 add
        assert c.dtype == np.float32
        lab = labels
        qualifies = (c == lab[v]) & (lab[u] < lab[v])
    violates = c < lab[v]
    return u, v, qualifies & live, violates & live


def chain_steps(pred):
    """Predecessor steps from every vertex to the end of its chain (a vertex that is its own
    predecessor or has none: the source, an orphan, an unreached vertex), and that end."""
    pred = np.asarray(pred, np.int64)
    n = len(pred)
    end = np.where((pred < 0) | (pred == np.arange(n)), np.arange(n), -1)
    steps = np.where(end >= 0, 0, -1)
    for start in range(n):
        walked, v = [], start
        while end[v] < 0:
            walked.append(v)
            v = pred[v]
        for i, x in enumerate(reversed(walked)):
            end[x], steps[x] = end[v], steps[v] + i + 1
    return steps, end


def doubling_rounds(pred):
    """grx_stats::iterations of a call with d_hops: ceil(log2(L)), 0 for L <= 1."""
    steps, _ = chain_steps(pred)
    longest = int(steps.max()) if len(steps) else 0
    return (longest - 1).bit_length() if longest > 1 else 0


def tree(ap, aj, aw, labels, source):
    """-> dict: pred (int32), hops (int32), orphans, violations, reached."""
    labels = np.asarray(labels)
    n = len(ap) - 1
    u, v, qualifies, violates = entries(ap, aj, aw, labels)
    best = np.full(n, NONE, np.int64)
    np.minimum.at(best, v[qualifies], u[qualifies])
    reached = labels != (INT_UNREACHED if labels.dtype.kind == "i" else FLT_UNREACHED)
    pred = np.where(~reached, -1, np.where(best == NONE, -2, best))
    pred[source] = source
    # hops: every predecessor has a strictly smaller label, so label order settles it before its children
    hops = np.full(n, -1, np.int64)
    hops[source] = 0
    keys = labels.astype(np.float64)
    for x in np.argsort(keys, kind="stable"):
        if x != source and pred[x] >= 0 and hops[pred[x]] >= 0:
            hops[x] = hops[pred[x]] + 1
    return {"pred": pred.astype(np.int32), "hops": hops.astype(np.int32), "orphans": int((pred == -2).sum()),
            "violations": int(violates.sum()), "reached": int(reached.sum())}


def path(pred, target):
    """The chain from `target` back to a self-predecessor, reversed; [] when it does not end at one."""
    walked, v = [int(target)], int(target)
    for _ in range(len(pred)):
        if pred[v] == v:
            return walked[::-1]
        if pred[v] < 0:
            return []
        v = int(pred[v])
        walked.append(v)
    return []
