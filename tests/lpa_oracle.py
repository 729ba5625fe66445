"""Semi-synchronous label propagation over the colour classes of `colouring` (color_oracle.py), and
the modularity of a labelling, in plain numpy.  The definition (include/essentials_amd.h): label[v]
= v; a sweep takes the colour classes in order, and a vertex of a class counts, per label, the
entries (v, u) of its row with u != v -- a repeated entry each time --, keeps its label when its
count is the largest (or when there is no such entry) and takes the label of smallest fmix32 among
the largest otherwise; the run stops after the first sweep that changes nothing, or after
max_sweeps.  The dirty rule: a vertex decides only while its flag is set and clears it, and a vertex
that changes sets the flag of every other vertex in its row.  `sequential` is that, vertex by
vertex; `communities` gets the same answer class by class, vectorised, and is what the GPU tests
compare against.  Both return (canonical int32 labels: the smallest vertex id with the same final
label; the number of communities; the sweeps; the changes per sweep; (row entries read by deciding
vertices, row entries read by changed vertices that mark their neighbours))."""
import numpy as np

from color_oracle import colouring, csr, fmix32, mtx_csr, simple_csr  # noqa: F401  (re-exported for the tests)


def _canonical(label):
    n = len(label)
    first = np.full(n, n, np.int64)
    np.minimum.at(first, label, np.arange(n, dtype=np.int64))
    out = first[label]
    return out.astype(np.int32), int((out == np.arange(n)).sum())


def sequential(ap, aj, max_sweeps=0, all_rows=False):
    ap = np.asarray(ap, np.int64)
    aj = np.asarray(aj, np.int64)
    n = len(ap) - 1
    if n == 0:
        return np.zeros(0, np.int32), 0, 0, [], (0, 0)
    color = colouring(ap, aj)[0].astype(np.int64)
    order = np.lexsort((np.arange(n), color))  # by (colour, id)
    h = fmix32(np.arange(n))
    label = np.arange(n, dtype=np.int64)
    dirty = np.ones(n, bool)
    changes, decided, marked = [], 0, 0
    while True:
        changed = 0
        for v in order:
            row = aj[ap[v]:ap[v + 1]]
            if len(row) == 0 or not (all_rows or dirty[v]):
                continue
            decided += len(row)
            dirty[v] = False
            count = {}
            for u in row:
                if u != v:
                    count[label[u]] = count.get(label[u], 0) + 1
            if not count:
                continue
            best = max(count.values())
            if count.get(label[v], 0) == best:
                continue
            label[v] = min((l for l, c in count.items() if c == best), key=lambda l: int(h[l]))
            changed += 1
            if not all_rows:
                marked += len(row)
                dirty[row[row != v]] = True
        changes.append(changed)
        if changed == 0 or len(changes) == max_sweeps:
            break
    out, count = _canonical(label)
    return out, count, len(changes), changes, (decided, marked)


def communities(ap, aj, max_sweeps=0, all_rows=False):
    ap = np.asarray(ap, np.int64)
    aj = np.asarray(aj, np.int64)
    n = len(ap) - 1
    if n == 0:
        return np.zeros(0, np.int32), 0, 0, [], (0, 0)
    color, num_colors, _ = colouring(ap, aj)
    color = color.astype(np.int64)
    deg = np.diff(ap)
    order = np.lexsort((np.arange(n), color))
    starts = np.searchsorted(color[order], np.arange(num_colors + 1))
    h = fmix32(np.arange(n)).astype(np.int64)
    label = np.arange(n, dtype=np.int64)
    dirty = np.ones(n, bool)
    changes, decided, marked = [], 0, 0
    while True:
        changed = 0
        for c in range(num_colors):
            vs = order[starts[c]:starts[c + 1]]
            vs = vs[(deg[vs] > 0) & (True if all_rows else dirty[vs])]
            if len(vs) == 0:
                continue
            lens = deg[vs]
            total = int(lens.sum())
            decided += total
            dirty[vs] = False
            slot = np.repeat(np.arange(len(vs)), lens)
            at = np.repeat(ap[vs] - (np.cumsum(lens) - lens), lens) + np.arange(total)
            u = aj[at]
            keep = u != vs[slot]
            pair, cnt = np.unique(slot[keep] * n + label[u[keep]], return_counts=True)
            if len(pair) == 0:
                continue
            s, l = pair // n, pair % n
            best = np.zeros(len(vs), np.int64)
            np.maximum.at(best, s, cnt)
            own = np.zeros(len(vs), np.int64)
            mine = l == label[vs[s]]
            own[s[mine]] = cnt[mine]
            top = cnt == best[s]
            # per slot the maximum of smallest hash: sort by (slot, hash) and take each slot's first
            ts, tl = s[top], l[top]
            by = np.lexsort((h[tl], ts))
            ts, tl = ts[by], tl[by]
            head = np.ones(len(ts), bool)
            head[1:] = ts[1:] != ts[:-1]
            choice = np.full(len(vs), -1, np.int64)
            choice[ts[head]] = tl[head]
            move = (best > 0) & (own != best)
            changed += int(move.sum())
            label[vs[move]] = choice[move]
            if not all_rows and move.any():
                marked += int(lens[move].sum())
                hit = move[slot] & keep
                dirty[u[hit]] = True
        changes.append(changed)
        if changed == 0 or len(changes) == max_sweeps:
            break
    out, count = _canonical(label)
    return out, count, len(changes), changes, (decided, marked)


def inside_entries(ap, aj, label):
    """The entries whose two ends carry the same label."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    col = np.asarray(aj, np.int64)[: len(row)]
    label = np.asarray(label, np.int64)
    return int((label[row] == label[col]).sum())


def modularity_parts(ap, aj, label):
    """(I, S, Q) in Python integers and the one float expression of the contract."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    e = int(ap[-1]) if n else 0
    label = np.asarray(label, np.int64)
    i = inside_entries(ap, aj, label)
    tot = np.zeros(max(n, 1), np.int64)
    np.add.at(tot, label, np.diff(ap))
    s = sum(int(t) * int(t) for t in tot[tot > 0])
    q = 0.0 if e == 0 else float(i) / float(e) - float(s) / (float(e) * float(e))
    return i, s, q
