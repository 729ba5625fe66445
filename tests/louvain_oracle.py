"""Louvain community detection as include/essentials_amd.h defines it (grx_louvain), in plain numpy
and exact integers.  A level graph is a symmetric CSR with integer weights; level 0 is the caller's
CSR with weight 1 per entry, a repeated entry counting each time.  A phase starts from label[v] = v
and tot[c] = k(c), colours the level graph's pattern CSR with `colouring` (color_oracle.py) and
sweeps the colour classes in order: every vertex of a class decides from label and tot as they
stand when its class begins, gain(c) = k_vc * E - k(v) * (tot[c] - k(v) [c == label[v]]), and moves
to the label of largest gain (smallest fmix32 among equals) when that beats its own label's gain.
After a sweep N = I * E - S is evaluated; a sweep without moves ends the phase, a sweep that does
not raise N is undone and ends the phase.  The communities of a phase that kept a move become the
next level's vertices, numbered by ascending smallest original vertex id.

`sequential` states a class's decisions vertex by vertex; `communities` is vectorised class by
class and is what the GPU tests compare against.  Both return (canonical int32 labels: the smallest
original vertex id of the same final community; the number of communities; Q; the levels = phases
run; the moves kept per sweep; per phase (n_L, entries of the level graph)).  `trace`, a list,
receives per phase a dict with the scores N before the phase and after every sweep."""
import numpy as np

from color_oracle import colouring, csr, fmix32, mtx_csr, simple_csr  # noqa: F401  (re-exported for the tests)
from lpa_oracle import modularity_parts


def _decide_sequential(vs, ap, aj, aw, k, label, tot, e, h):
    out = label[vs].copy()
    for i, v in enumerate(vs):
        v = int(v)
        kvc = {}
        for at in range(int(ap[v]), int(ap[v + 1])):
            u = int(aj[at])
            if u != v:
                c = int(label[u])
                kvc[c] = kvc.get(c, 0) + int(aw[at])
        own = int(label[v])
        kv = int(k[v])

        def gain(c):
            return kvc.get(c, 0) * e - kv * (int(tot[c]) - (kv if c == own else 0))

        others = [c for c in kvc if c != own]
        if not others:
            continue
        best = max(gain(c) for c in others)
        if best > gain(own):
            out[i] = min((c for c in others if gain(c) == best), key=lambda c: int(h[c]))
    return out


def _decide_vectorised(vs, ap, aj, aw, k, label, tot, e, h):
    n = len(ap) - 1
    out = label[vs].copy()
    lens = ap[vs + 1] - ap[vs]
    total = int(lens.sum())
    slot = np.repeat(np.arange(len(vs)), lens)
    at = np.repeat(ap[vs] - (np.cumsum(lens) - lens), lens) + np.arange(total)
    u = aj[at]
    keep = u != vs[slot]
    pair, inv = np.unique(slot[keep] * n + label[u[keep]], return_inverse=True)
    if len(pair) == 0:
        return out
    kvc = np.zeros(len(pair), np.int64)
    np.add.at(kvc, inv.reshape(-1), aw[at][keep])
    s, c = pair // n, pair % n
    v = vs[s]
    mine = c == label[v]
    gain = kvc * e - k[v] * (tot[c] - np.where(mine, k[v], 0))
    own_kvc = np.zeros(len(vs), np.int64)
    own_kvc[s[mine]] = kvc[mine]
    own_gain = own_kvc * e - k[vs] * (tot[label[vs]] - k[vs])
    so, co, go = s[~mine], c[~mine], gain[~mine]
    if len(so) == 0:
        return out
    low = np.iinfo(np.int64).min
    best = np.full(len(vs), low, np.int64)
    np.maximum.at(best, so, go)
    top = go == best[so]
    ts, tc = so[top], co[top]
    by = np.lexsort((h[tc], ts))
    ts, tc = ts[by], tc[by]
    head = np.ones(len(ts), bool)
    head[1:] = ts[1:] != ts[:-1]
    choice = np.full(len(vs), -1, np.int64)
    choice[ts[head]] = tc[head]
    move = (best > low) & (best > own_gain)
    out[move] = choice[move]
    return out


def _score(ap, aj, aw, label, tot, e):
    """N = I * E - S as a Python integer."""
    row = np.repeat(np.arange(len(ap) - 1, dtype=np.int64), np.diff(ap))
    inside = int(aw[label[row] == label[aj]].sum())
    return inside * e - sum(int(t) * int(t) for t in tot[tot > 0])


def _phase(ap, aj, aw, e, decide, record):
    """One phase on a level graph -> (label, moves kept per sweep)."""
    n = len(ap) - 1
    k = np.zeros(n, np.int64)
    np.add.at(k, np.repeat(np.arange(n, dtype=np.int64), np.diff(ap)), aw)
    color, num_colors, _ = colouring(ap, aj)
    color = color.astype(np.int64)
    order = np.lexsort((np.arange(n), color))
    starts = np.searchsorted(color[order], np.arange(num_colors + 1))
    h = fmix32(np.arange(n)).astype(np.int64)
    label = np.arange(n, dtype=np.int64)
    tot = k.copy()
    score = _score(ap, aj, aw, label, tot, e)
    record["scores"] = [score]
    record["undone"] = False
    kept = []
    while True:
        before = (label.copy(), tot.copy())
        moves = 0
        for c in range(num_colors):
            vs = order[starts[c]:starts[c + 1]]
            vs = vs[ap[vs + 1] > ap[vs]]
            if len(vs) == 0:
                continue
            new = decide(vs, ap, aj, aw, k, label, tot, e, h)
            moved = new != label[vs]
            if moved.any():
                mv, to = vs[moved], new[moved]
                np.subtract.at(tot, label[mv], k[mv])
                np.add.at(tot, to, k[mv])
                label[mv] = to
                moves += int(moved.sum())
        if moves == 0:
            kept.append(0)
            break
        after = _score(ap, aj, aw, label, tot, e)
        if after <= score:
            label, tot = before
            record["undone"] = True
            kept.append(0)
            break
        score = after
        record["scores"].append(score)
        kept.append(moves)
    return label, kept


def _aggregate(ap, aj, aw, label):
    """(new id per level vertex, the next level graph): the communities by ascending smallest member."""
    n = len(ap) - 1
    names, first = np.unique(label, return_index=True)
    rank_of = np.zeros(n, np.int64)
    rank_of[names[np.argsort(first, kind="stable")]] = np.arange(len(names))
    nid = rank_of[label]
    m = len(names)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    key, inv = np.unique(nid[row] * m + nid[aj], return_inverse=True)
    w = np.zeros(len(key), np.int64)
    np.add.at(w, inv.reshape(-1), aw)
    nap = np.zeros(m + 1, np.int64)
    nap[1:] = np.cumsum(np.bincount(key // m, minlength=m))
    return nid, (nap, key % m, w)


def _run(ap, aj, max_phases, decide, trace):
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    if n == 0:
        return np.zeros(0, np.int32), 0, 0.0, 0, [], []
    aj = np.asarray(aj, np.int64)[: int(ap[-1])]
    e = int(ap[-1])
    level = (ap, aj, np.ones(e, np.int64))
    comm = np.arange(n, dtype=np.int64)
    kept, shapes, levels = [], [], 0
    while True:
        record = {}
        shapes.append((len(level[0]) - 1, len(level[1])))
        label, sweeps = _phase(*level, e, decide, record)
        kept += sweeps
        levels += 1
        if trace is not None:
            trace.append(record)
        if not any(sweeps):
            break
        nid, level = _aggregate(*level, label)
        comm = nid[comm]
        if levels == max_phases:
            break
    first = np.full(int(comm.max()) + 1, n, np.int64)
    np.minimum.at(first, comm, np.arange(n, dtype=np.int64))
    out = first[comm].astype(np.int32)
    q = modularity_parts(ap, aj, out)[2]
    return out, int((out == np.arange(n)).sum()), q, levels, kept, shapes


def sequential(ap, aj, max_phases=0, trace=None):
    return _run(ap, aj, max_phases, _decide_sequential, trace)


def communities(ap, aj, max_phases=0, trace=None):
    return _run(ap, aj, max_phases, _decide_vectorised, trace)


def level_graph(ap, aj, phases):
    """The weighted level graph (ap, aj, aw) after `phases` phases that kept moves, for the tests."""
    ap = np.asarray(ap, np.int64)
    e = int(ap[-1])
    level = (ap, np.asarray(aj, np.int64)[:e], np.ones(e, np.int64))
    for _ in range(phases):
        label, sweeps = _phase(*level, e, _decide_vectorised, {})
        if not any(sweeps):
            break
        level = _aggregate(*level, label)[1]
    return level


# a symmetrised multigraph of 8 vertices whose first phase keeps a sweep of 6 moves and undoes one of 2
UNDO_EDGES = [[1, 3], [1, 3], [1, 6], [1, 5], [0, 2], [0, 3], [0, 3], [1, 3], [1, 3], [1, 4], [0, 2], [1, 7], [1, 4],
              [1, 4], [0, 5], [1, 5], [0, 4]]


def planted(blocks=20, size=25, p_in=0.4, p_out=0.01, seed=2):
    """(ap, aj, block of every vertex): one draw per pair of the upper triangle."""
    n = blocks * size
    block = np.arange(n) // size
    a, b = np.triu_indices(n, 1)
    hit = np.random.default_rng(seed).random(len(a)) < np.where(block[a] == block[b], p_in, p_out)
    ap, aj = csr(n, np.stack([a[hit], b[hit]], 1))
    return ap, aj, block
