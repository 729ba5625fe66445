"""Strongly connected components of a CSR in plain numpy and Python (the GPU machine may lack scipy
and networkx): Tarjan's algorithm with an explicit stack, no recursion.  The label of a vertex is
the smallest vertex id of its component, the convention of cc_oracle.components, so on a symmetric
CSR the two agree.  Self loops and repeated entries change nothing."""
import numpy as np

import cc_oracle
from tc_oracle import csr, mtx_csr  # noqa: F401  (re-exported for the tests)


def strong_components(ap, aj):
    """(int32 labels: the smallest vertex id of each vertex's strongly connected component, number
    of components)."""
    ap = np.asarray(ap, np.int64).tolist()
    aj = np.asarray(aj, np.int64).tolist()
    n = len(ap) - 1
    index = [-1] * n  # discovery number
    low = [0] * n
    on_stack = [False] * n
    label = [0] * n
    stack, count, clock = [], 0, 0
    for root in range(n):
        if index[root] >= 0:
            continue
        index[root] = low[root] = clock
        clock += 1
        stack.append(root)
        on_stack[root] = True
        work = [(root, ap[root])]  # (vertex, next entry of its row)
        while work:
            u, e = work[-1]
            if e < ap[u + 1]:
                work[-1] = (u, e + 1)
                w = aj[e]
                if index[w] < 0:
                    index[w] = low[w] = clock
                    clock += 1
                    stack.append(w)
                    on_stack[w] = True
                    work.append((w, ap[w]))
                elif on_stack[w] and index[w] < low[u]:
                    low[u] = index[w]
                continue
            work.pop()
            if work and low[u] < low[work[-1][0]]:
                low[work[-1][0]] = low[u]
            if low[u] == index[u]:  # u is the root of a component: everything above it on the stack
                at = len(stack) - 1
                while stack[at] != u:
                    at -= 1
                members = stack[at:]
                del stack[at:]
                smallest = min(members)
                for w in members:
                    on_stack[w] = False
                    label[w] = smallest
                count += 1
    return np.asarray(label, np.int32), count


def _ring(first, size, step=1):
    return [(first + i, first + (i + step) % size) for i in range(size)]


def _known():
    k = {}
    k["empty"] = (0, [], False, [])
    k["isolated"] = (9, [], False, list(range(9)))
    k["self_loops_only"] = (4, [(0, 0), (2, 2), (2, 2), (3, 3)], False, [0, 1, 2, 3])
    k["two_cycle"] = (2, [(0, 1), (1, 0)], False, [0, 0])
    k["directed_chain"] = (40, [(i, i + 1) for i in range(39)], False, list(range(40)))
    k["ring_forwards"] = (9, _ring(0, 9), False, [0] * 9)
    k["ring_backwards"] = (9, _ring(0, 9, -1), False, [0] * 9)
    two_rings = _ring(0, 5) + _ring(5, 5)
    k["two_rings_2_to_7"] = (10, two_rings + [(2, 7)], False, [0] * 5 + [5] * 5)
    k["two_rings_7_to_2"] = (10, two_rings + [(7, 2)], False, [0] * 5 + [5] * 5)
    k["two_rings_both_ways"] = (10, two_rings + [(2, 7), (8, 1)], False, [0] * 10)
    # evens and odds: 0 -> 2 -> ... -> 10 -> 0 and 1 -> 3 -> ... -> 9 -> 1, joined one way by 0 -> 1
    k["interleaved_rings"] = (11, [(i, i + 2) for i in range(9)] + [(10, 0), (9, 1), (0, 1)], False,
                              [i % 2 for i in range(11)])
    k["bow_tie"] = (7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 2), (4, 5), (5, 6)], False, [0, 1, 2, 2, 2, 5, 6])
    k["out_star_evens_return"] = (20, [(7, i) for i in range(20) if i != 7] + [(i, 7) for i in range(0, 20, 2)], False,
                                  [0 if i % 2 == 0 or i == 7 else i for i in range(20)])
    k["complete5_every_entry_three_times"] = (6, [(a, b) for a in range(5) for b in range(5) if a != b] * 3, False,
                                              [0] * 5 + [5])
    k["diamond_dag"] = (4, [(0, 1), (0, 2), (1, 3), (2, 3)], False, [0, 1, 2, 3])
    # symmetric: every edge runs both ways, and the labels are the weak ones
    for name in ("two_cliques", "k4_every_edge_three_times", "interleaved"):
        n, edges, both, want = cc_oracle.KNOWN[name]
        assert both
        k["symmetric_" + name] = (n, edges, True, want)
    return k


# name -> (V, edge list, add both directions, labels)
KNOWN = _known()


def known_csr(name):
    n, edges, both, want = KNOWN[name]
    ap, aj = csr(n, np.asarray(edges, np.int64).reshape(-1, 2), symmetric=both)
    return ap, aj, np.asarray(want, np.int32)
