#!/usr/bin/env python3
"""Time spatial_graph at 10^6 points (side x side, default 1000 x 1000): a unit lattice at max_dist 1.5 (the 3 x 3
neighbourhood GCNMF's tests use) in spatial order and with the labels randomly permuted (the selection is by index, so the
same geometry under other names), uniform random points on the same square at max_dist 2.5, and the all-in-range case
(max_dist above the extent: every point a candidate of every other, the scan ends at max_k).  max_k = 100.  Times are
whole one-shot calls (upload, cell list, both passes, download), median of `reps`.  Also the test-side numpy
restatement's CPU time on a sample of columns, labelled as such (it is not the reference, which needs R).
Prints one JSON line.
usage: spatial_graph_rate.py [side] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import singlet_amd as sa  # noqa: E402
import spatial_graph_restatement as sr  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = side * side
MAX_K = 100

rng = np.random.default_rng(0)
x, y = sr.lattice(side)
perm = rng.permutation(n)
rx, ry = rng.random(n) * side, rng.random(n) * side
cases = {"lattice": (x, y, 1.5), "lattice_shuffled": (x[perm], y[perm], 1.5), "random": (rx, ry, 2.5),
         "all_in_range": (rx, ry, 2.0 * side)}


def timed(fn):
    fn()   # warm-up (pool, code objects)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return out, 1e3 * float(np.median(ts))


res = {"points": n, "max_k": MAX_K, "reps": reps}
for name, (cx, cy, md) in cases.items():
    g, t = timed(lambda: sa.spatial_graph(cx, cy, md, MAX_K))
    # bytes out: i (4) and x (8) per entry, downloaded; in: c1, c2 (16 per point) uploaded
    res[name] = {"max_dist": md, "ms": t, "nnz": int(g.p[-1]), "entries_per_s": g.p[-1] / (t / 1e3),
                 "d2h_GB": 12.0 * g.p[-1] / 1e9, "h2d_GB": 16.0 * n / 1e9}

# the restatement on a sample of columns (CPU numpy, not the reference)
cl = sr.CellList(rx, ry, 2.5, MAX_K)
pts = rng.choice(n, 2000, replace=False)
t = time.perf_counter()
for c in pts:
    cl.column(int(c))
res["restatement_cpu_s_per_1000_columns_random"] = (time.perf_counter() - t) / 2.0
print(json.dumps(res))
