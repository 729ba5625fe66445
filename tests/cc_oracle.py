"""Connected components of a CSR (weakly connected on a directed one) in plain numpy (the GPU
machine may lack scipy and networkx): min-label hooking with pointer jumping.  Every entry (u, v)
lowers the labels of u, of v and of the vertices their old labels name to the smaller of the two
labels (np.minimum.at), then label = label[label] until stable; repeated until nothing changes.
A label never exceeds its vertex and always names a vertex of the same component, so at the fixed
point it is the component's smallest vertex id."""
import numpy as np

from tc_oracle import csr, mtx_csr  # noqa: F401  (re-exported for the tests)


def components(ap, aj):
    """(int32 labels: the smallest vertex id of each vertex's component, number of components)."""
    ap = np.asarray(ap, np.int64)
    n = len(ap) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ap))
    dst = np.asarray(aj, np.int64)[: len(src)]
    label = np.arange(n, dtype=np.int64)
    while True:
        ls, ld = label[src], label[dst]
        open_ = ls != ld  # the other entries would change nothing in this pass
        if not open_.any():
            break
        low = np.minimum(ls[open_], ld[open_])
        for at in (src[open_], dst[open_], ls[open_], ld[open_]):
            np.minimum.at(label, at, low)
        while True:
            nxt = label[label]
            if (nxt == label).all():
                break
            label = nxt
    return label.astype(np.int32), int((label == np.arange(n)).sum())


def _clique(first, size):
    return [(first + a, first + b) for a in range(size) for b in range(a + 1, size)]


def _known():
    k = {}
    k["empty"] = (0, [], True, [])
    k["isolated"] = (9, [], True, list(range(9)))
    k["only_a_self_loop"] = (3, [(1, 1)], False, [0, 1, 2])
    for n in (2, 5, 12):
        k[f"complete{n}"] = (n, _clique(0, n), True, [0] * n)
    k["path"] = (30, [(i, i + 1) for i in range(29)], True, [0] * 30)
    k["cycle"] = (9, [(i, (i + 1) % 9) for i in range(9)], True, [0] * 9)
    k["star"] = (30, [(0, i) for i in range(1, 30)], True, [0] * 30)
    k["star_hub_last"] = (30, [(29, i) for i in range(29)], True, [0] * 30)
    k["two_cliques"] = (9, _clique(0, 4) + _clique(4, 5), True, [0] * 4 + [4] * 5)
    k["two_cliques_bridge"] = (9, _clique(0, 4) + _clique(4, 5) + [(3, 4)], True, [0] * 9)
    k["k4_every_edge_three_times"] = (6, _clique(1, 4) * 3, True, [0, 1, 1, 1, 1, 5])
    k["directed_chain"] = (40, [(i, i + 1) for i in range(39)], False, [0] * 40)
    k["directed_chain_backwards"] = (40, [(i + 1, i) for i in range(39)], False, [0] * 40)
    k["directed_in_star"] = (20, [(i, 7) for i in range(20) if i != 7], False, [0] * 20)
    k["directed_out_star"] = (20, [(7, i) for i in range(20) if i != 7], False, [0] * 20)
    # evens and odds: the smallest ids 0 and 1 are neighbours in the numbering, not in the graph
    k["interleaved"] = (11, [(i, i + 2) for i in range(9)], True, [i % 2 for i in range(11)])
    k["interleaved_directed"] = (11, [(i + 2, i) for i in range(9)], False, [i % 2 for i in range(11)])
    return k


# name -> (V, edge list, add both directions, labels)
KNOWN = _known()


def known_csr(name):
    n, edges, both, want = KNOWN[name]
    ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2), symmetric=both)
    return ap, aj, np.asarray(want, np.int32)
