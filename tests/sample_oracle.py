"""Oracle of grx_neighbor_sample: the definition of include/essentials_amd.h followed literally, one hop,
one row and one attempt at a time, in Python integers.  The checker, never the thing shipped."""
import numpy as np

from walk_oracle import M64, chi_square, csr, draw, mix64, mtx_csr, pick_uniform  # noqa: F401 (re-exported)

ALL, INCLUDE, EXCLUDE = 0, 1, 2
MAX_FANOUT = 1024


def sample_plan(d, k):
    """-> (mode, m): what a row of d entries does under fan-out k (-1: every entry)."""
    if k < 0 or d <= k:
        return ALL, 0
    if 2 * k <= d:
        return INCLUDE, k
    return EXCLUDE, d - k


def attempt_bound(m):
    return 64 * m + 1024


def candidate(seed, v, hop, a, d):
    """x_a of row v in hop `hop`: r(v, hop, a) scaled to [0, d)."""
    return pick_uniform(draw(seed, v, hop, a), d)


def sample_row(seed, hop, v, d, k):
    """-> (the chosen positions of the row, ascending; A, the candidates drawn: 0 for an all-row)."""
    mode, m = sample_plan(d, k)
    if mode == ALL:
        return list(range(d)), 0
    stream = mix64((seed & M64) ^ mix64(v))
    found, a = set(), 0
    while len(found) < m:
        assert a < attempt_bound(m), "the attempt bound"
        found.add(pick_uniform(mix64((stream + (hop << 32) + a) & M64), d))
        a += 1
    if mode == INCLUDE:
        return sorted(found), a
    return [p for p in range(d) if p not in found], a


def neighbor_sample(ap, aj, seeds, fanouts, seed):
    """-> dict: nodes, node_offsets (len(fanouts) + 2), src, dst (local ids), entries, edge_offsets
    (len(fanouts) + 1), and the pinned stats: iterations (hops that expanded a vertex), slots (vertices
    expanded per hop), attempts (the sum of A) and expanded (attempts + the length of every all-row)."""
    ap, aj = np.asarray(ap, np.int64), np.asarray(aj, np.int64)
    n = len(ap) - 1
    seeds = range(n) if seeds is None else [int(s) for s in np.atleast_1d(np.asarray(seeds, np.int64))]
    local, nodes = {}, []
    for s in seeds:
        if s not in local:
            local[s] = len(nodes)
            nodes.append(s)
    node_offsets, edge_offsets = [0, len(nodes)], [0]
    src, dst_global, entries, slots = [], [], [], []
    attempts = expanded = iterations = 0
    for hop, k in enumerate(fanouts, start=1):
        assert k == -1 or 1 <= k <= MAX_FANOUT
        frontier = nodes[node_offsets[-2]:node_offsets[-1]]
        slots.append(len(frontier))
        iterations += 1 if frontier else 0
        named = set()
        for v in frontier:
            lo, d = int(ap[v]), int(ap[v + 1] - ap[v])
            positions, A = sample_row(seed, hop, v, d, k)
            attempts += A
            expanded += A if A else d
            for p in positions:
                src.append(local[v])
                entries.append(lo + p)
                dst_global.append(int(aj[lo + p]))
                named.add(int(aj[lo + p]))
        for u in sorted(named):
            if u not in local:
                local[u] = len(nodes)
                nodes.append(u)
        node_offsets.append(len(nodes))
        edge_offsets.append(len(src))
    return {"nodes": np.asarray(nodes, np.int32), "node_offsets": node_offsets,
            "src": np.asarray(src, np.int32), "dst": np.asarray([local[u] for u in dst_global], np.int32),
            "entries": np.asarray(entries, np.int32), "edge_offsets": edge_offsets,
            "iterations": iterations, "slots": slots, "attempts": attempts, "expanded": expanded}
