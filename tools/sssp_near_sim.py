#!/usr/bin/env python3
"""Host simulation behind the near / far selection of grx_sssp: how many edge
relaxations frontier SSSP spends per reached edge, with and without deferring the far part of a
wide pending set.  CPU only: numpy and the oracle's R-MAT generator (the bench's graph family:
symmetric, edge factor 16, seed 1, weight seed 7, weights 1..64).

    python tools/sssp_near_sim.py                       # the table of DESIGN.md: scale 20 and 18
    python tools/sssp_near_sim.py --scale 18 --frac 0.5 0.33 --sources 0 1234

Rounds are SYNCHRONOUS (every relaxation of a round reads the distances of the round's start), which
the engine's are not: it reads labels live, so its plain run already does better than the figures in
the first column.

  plain      every vertex lowered in round r is expanded in round r + 1
  frac f     pending = lowered since last expanded; a round expands the pending vertices with
             distance <= T, T the smallest distance at which they hold at least the share f of the
             pending edge work; once the pending work is below --min-work (default |E| / 64, the label
             scan threshold's share of R-MAT-22) everything pending is expanded
  --codes    T is chosen among the engine's 4096 distance codes (8 per octave) instead of among the
             exact distances

Distances are asserted bit-equal between all variants and the oracle's heap search.

What it prints, relaxations / reached edges (rounds), with the defaults:

    scale 20, source 0        1.74 (8)   frac 0.5 1.17 (11)   frac 0.33 1.05 (12)
    scale 20, source 715782   2.37 (10)           1.44 (12)             1.26 (15)
    scale 20, source 802689   1.87 (9)            1.23 (12)             1.08 (14)
    scale 20, source 90402    2.32 (9)            1.49 (12)             1.26 (14)
    scale 18, 4 sources       1.75-2.60 (8-10)    1.18-1.58 (10-13)     1.05-1.35 (12-14)

With --min-work 1 deferral goes on to the last vertex and the rounds grow by a tail of small ones.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.oracle import Oracle  # noqa: E402

FAR = np.float32(np.finfo(np.float32).max)


def code_of(d):
    """The engine's distance code: top 12 bits of the 2-byte upper bound of the ordered float bits."""
    bits = d.view(np.uint32) ^ np.uint32(0x80000000)     # distances are non-negative
    up = (bits >> np.uint32(16)) + ((bits & np.uint32(0xffff)) != 0)
    return np.minimum(up, 0xffff) >> 4


def expand(Ap, Aj, Ax, d, who):
    """One synchronous round from the vertices `who`: -> (new distances, lowered mask, edges relaxed)."""
    starts, counts = Ap[who], (Ap[who + 1] - Ap[who])
    total = int(counts.sum())
    if total == 0:
        return d, np.zeros(len(d), bool), 0
    # edge ids of all rows of `who`, concatenated
    offs = np.repeat(starts - np.concatenate(([0], np.cumsum(counts)[:-1])), counts) + np.arange(total)
    cand = np.repeat(d[who], counts) + Ax[offs]           # float32 + float32, as the engine adds
    new = d.copy()
    np.minimum.at(new, Aj[offs], cand)
    return new, new < d, total


def run(Ap, Aj, Ax, source, frac=None, min_work=0, codes=False):
    n = len(Ap) - 1
    deg = np.diff(Ap).astype(np.int64)
    d = np.full(n, FAR, np.float32)
    d[source] = 0
    pending = np.zeros(n, bool)
    pending[source] = True
    relaxed = rounds = 0
    while pending.any():
        who = np.flatnonzero(pending)
        work = deg[who]
        total = int(work.sum())
        if frac is not None and total >= max(min_work, 1):
            key = code_of(d[who]) if codes else d[who]
            order = np.argsort(key, kind="stable")
            cum = np.cumsum(work[order])
            at = int(np.searchsorted(cum, max(1, int(frac * total))))
            who = who[key <= key[order[min(at, len(order) - 1)]]]
        pending[who] = False
        d, lowered, e = expand(Ap, Aj, Ax, d, who)
        pending |= lowered
        relaxed += e
        rounds += 1
    return d, relaxed, rounds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, nargs="*", default=[20, 18])
    ap.add_argument("--frac", type=float, nargs="*", default=[0.5, 0.33])
    ap.add_argument("--sources", type=int, nargs="*", default=None,
                    help="default: 0 and three seeded random vertices with edges")
    ap.add_argument("--min-work", type=int, default=None, help="default: |E| / 64")
    ap.add_argument("--codes", action="store_true")
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
        print(f"scale {scale}: {n} vertices, {len(Aj)} edges, deferral ends below {min_work} edges of pending work"
              + (", thresholds among the engine's codes" if a.codes else ""))
        print("| source | plain | " + " | ".join(f"frac {f}" for f in a.frac) + " |")
        for s in sources:
            want, _ = o.sssp_heap(Ap, Aj, Ax, s)
            reached = int(deg[want != FAR].sum())
            cells = []
            for f in [None] + a.frac:
                d, relaxed, rounds = run(Ap, Aj, Ax, s, f, min_work, a.codes)
                assert (d.view(np.uint32) == want.view(np.uint32)).all(), (scale, s, f)
                cells.append(f"{relaxed / reached:.2f} ({rounds})")
            print(f"| {s} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
