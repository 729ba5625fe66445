#!/usr/bin/env python3
"""Host simulation behind the pulled rounds of grx_sssp: how many edges frontier
SSSP looks at per reached edge when the wide rounds of a weight-symmetric graph are pulled over rows
sorted by ascending weight, with a distance cut-off.  CPU only: numpy and the oracle's R-MAT generator
(the bench's graph family: symmetric, edge factor 16, seed 1, weight seed 7, weights 1..64).

    python tools/sssp_pull_sim.py                         # scale 18, four sources
    python tools/sssp_pull_sim.py --scale 20 --sources 0 --rounds

Rounds are SYNCHRONOUS and selected as tools/sssp_near_sim.py selects them (share 0.33, thresholds among
the engine's distance codes).  A round whose frontier holds `work` edges is PULLED when work > alpha x
the out-degree sum of the vertices still unreached: every vertex v with current label cur reads its
row from the lightest entry on and stops at the first entry of weight w with fl(dmin + w) >= cur, dmin
the smallest distance in the pending set; a lowered cur tightens the test.  v is not opened at all
when its lightest entry fails the test.  The comparison is made on the float32 SUM, which is monotone in
w, so the entries read are a prefix of the row and no skipped entry can carry a shorter path.

Distances are asserted bit-equal to oracle.sssp_heap for the weights 1..64 and for the same weights
x 0.1 and x 0.37 (float32 path sums that round).

What it prints: per source, edges looked at / reached edges for all push and for the hybrid; with
--rounds, per round: push work, or for a pulled round its work / entries examined / rows opened.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.oracle import Oracle  # noqa: E402
from sssp_near_sim import FAR, code_of, expand  # noqa: E402


def sort_rows(Ap, Aj, Ax):
    """Every row by ascending weight (stable): -> (neighbours, weights) under the same offsets."""
    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))
    order = np.lexsort((Ax, rows))
    return Aj[order], Ax[order]


def pull(Ap, Sj, Sx, d, dmin):
    """One synchronous pulled round: -> (new distances, lowered mask, entries examined, rows opened)."""
    deg = np.diff(Ap)
    cur = d.copy()
    has = np.flatnonzero(deg > 0)
    first = Sx[Ap[has]]
    active = has[(dmin + first).astype(np.float32) < cur[has]]
    opened, examined, j = len(active), 0, 0
    while len(active):
        at = Ap[active] + j
        w, u = Sx[at], Sj[at]
        go = (dmin + w).astype(np.float32) < cur[active]
        active, w, u = active[go], w[go], u[go]
        examined += len(active)
        with np.errstate(over="ignore"):
            through = np.where(d[u] != FAR, (d[u] + w).astype(np.float32), FAR)
        cur[active] = np.minimum(cur[active], through)
        j += 1
        active = active[deg[active] > j]
    return cur, cur < d, examined, opened


def run(Ap, Aj, Ax, source, alpha=None, frac=0.33, min_work=0, log=None):
    """alpha None: all push.  -> (distances, edges looked at, rounds, rounds pulled)."""
    n = len(Ap) - 1
    deg = np.diff(Ap).astype(np.int64)
    Sj, Sx = sort_rows(Ap, Aj, Ax)
    d = np.full(n, FAR, np.float32)
    d[source] = 0
    pending = np.zeros(n, bool)
    pending[source] = True
    looked = rounds = pulled = 0
    while pending.any():
        who = np.flatnonzero(pending)
        work = deg[who]
        total = int(work.sum())
        dmin = d[who].min()
        selected = rounds > 0 and total >= max(min_work, 1)   # the source's own round is never split
        if selected:
            key = code_of(d[who])
            order = np.argsort(key, kind="stable")
            cum = np.cumsum(work[order])
            at = int(np.searchsorted(cum, max(1, int(frac * total))))
            who = who[key <= key[order[min(at, len(order) - 1)]]]
        pending[who] = False
        round_work = int(deg[who].sum())
        unreached = int(deg[d == FAR].sum())
        if alpha is not None and rounds > 0 and round_work > alpha * unreached:
            d, lowered, examined, opened = pull(Ap, Sj, Sx, d, dmin)
            looked += examined
            pulled += 1
            if log is not None:
                log.append(f"    round {rounds}: pulled, work {round_work} examined {examined} rows opened {opened} "
                           f"unreached work {unreached} dmin {dmin:g}")
        else:
            d, lowered, e = expand(Ap, Aj, Ax, d, who)
            looked += e
            if log is not None:
                log.append(f"    round {rounds}: pushed, work {e} unreached work {unreached}")
        pending |= lowered
        rounds += 1
    return d, looked, rounds, pulled


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, nargs="*", default=[18])
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--sources", type=int, nargs="*", default=None,
                    help="default: 0 and three seeded random vertices with edges")
    ap.add_argument("--min-work", type=int, default=None, help="default: |E| / 64")
    ap.add_argument("--rounds", action="store_true", help="one line per round of the hybrid (weights 1..64)")
    a = ap.parse_args()
    o = Oracle()
    for scale in a.scale:
        n, Ap, Aj, Ax = o.rmat_csr(scale, 16, 1, 7, True)
        Aj, Ax = np.ascontiguousarray(Aj), np.ascontiguousarray(Ax)
        deg = np.diff(Ap)
        sources = a.sources
        if sources is None:
            rng = np.random.default_rng(scale)
            sources = [0] + [int(x) for x in rng.choice(np.flatnonzero(deg > 0), 3, replace=False)]
        min_work = a.min_work if a.min_work is not None else len(Aj) // 64
        print(f"scale {scale}: {n} vertices, {len(Aj)} edges, alpha {a.alpha}")
        print("| source | all push | hybrid push / sorted pull (rounds, pulled) |")
        for s in sources:
            for factor in (1.0, 0.1, 0.37):
                W = (Ax * np.float32(factor)).astype(np.float32)
                want, _ = o.sssp_heap(Ap, Aj, W, s)
                reached = int(deg[want != FAR].sum())
                log = [] if a.rounds and factor == 1.0 else None
                cells = []
                for alpha in (None, a.alpha):
                    d, looked, rounds, pulled = run(Ap, Aj, W, s, alpha, 0.33, min_work, log if alpha is not None else None)
                    assert (d.view(np.uint32) == want.view(np.uint32)).all(), (scale, s, factor, alpha)
                    cells.append(f"{looked / reached:.2f} ({rounds}, {pulled})")
                if factor == 1.0:
                    print(f"| {s} | " + " | ".join(cells) + " |", flush=True)
                    for line in log or ():
                        print(line)


if __name__ == "__main__":
    main()
