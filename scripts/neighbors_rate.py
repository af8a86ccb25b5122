#!/usr/bin/env python3
"""Time the spatial neighbour graphs on a side x side lattice (default 1000 x 1000 = 10^6 cells) at rank k (50), radius r
(4), k-param 20, jaccard, no max_dist pruning (FindLocalNeighbors' default 1/10 prunes every jaccard distance of a random
embedding): c_LKNN, and c_SNN on its pattern, in spatial order and with the cell labels
randomly permuted (the embedding and coordinates shuffled together: the same graph under other names, gathers out of
spatial order).  Times are whole one-shot calls (upload, validation, both passes, download), median of `reps`.  Also the
test-side numpy restatement's CPU time on a sample of points, labelled as such (it is not the reference, which needs R).
Prints one JSON line.
usage: neighbors_rate.py [side] [k] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import singlet_amd as sa  # noqa: E402
import local_neighbors_restatement as lr  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
n = side * side
R, KP, MD = 4.0, 20, 0.0

rng = np.random.default_rng(0)
x, y = lr.lattice(side)
m = np.asfortranarray(rng.random((k, n)) * (rng.random((k, n)) < 0.5))
perm = rng.permutation(n)
xs, ys, ms = x[perm], y[perm], np.asfortranarray(m[:, perm])


def timed(fn):
    fn()   # warm-up (pool, code objects)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return out, 1e3 * float(np.median(ts))


res = {"cells": n, "k": k, "radius": R, "k_param": KP, "metric": "jaccard", "max_dist": MD, "reps": reps}
for name, (mm, xx, yy) in (("spatial", (m, x, y)), ("shuffled", (ms, xs, ys))):
    knn, t_lknn = timed(lambda: sa.c_LKNN(mm, xx, yy, KP, R, "jaccard", True, MD, False, 0))
    knn.x = np.ones_like(knn.x)
    snn, t_snn = timed(lambda: sa.c_SNN(knn, 1 / 15, 0))
    r = {"lknn_ms": t_lknn, "snn_ms": t_snn, "knn_nnz": knn.nnz, "snn_nnz": snn.nnz}
    # bytes the LKNN candidate tests gather: each point reads its candidates' k floats (3 x 3 buckets of side ~r, ~13^2
    # candidates) -- from L2 / MALL mostly in spatial order; H2D of m (8 k n bytes) is part of the call
    cand = 13 * 13
    r["lknn_gathered_GB"] = 4.0 * k * cand * n / 1e9
    r["lknn_gathered_TBps"] = r["lknn_gathered_GB"] / t_lknn
    r["lknn_h2d_GB"] = 8.0 * k * n / 1e9
    # SNN: each column gathers the column lists of its rows (~knn_nnz / n rows of ~that many entries), twice (two passes)
    per = knn.nnz / n
    r["snn_gathered_GB"] = 2 * 4.0 * per * per * n / 1e9
    r["snn_gathered_TBps"] = r["snn_gathered_GB"] / t_snn
    res[name] = r

# the restatement on a sample (CPU numpy, not the reference)
pts = rng.choice(n, 2000, replace=False)
t = time.perf_counter()
lr.lknn_grid(m, x, y, KP, R, "jaccard", True, MD, points=pts)
res["restatement_cpu_s_per_1000_points"] = (time.perf_counter() - t) / 2.0
res["hbm_peak_TBps"] = 8.0
print(json.dumps(res))
