#!/usr/bin/env python3
"""Spatially variable genes of a synthetic tissue by Moran's I (find_spatially_variable_features): a grid of cells, a few genes
expressed in a rectangular domain each, and the other genes with the same kind of values but their cells shuffled.  The graph
is spatial_graph of the grid coordinates; the planted genes must rank first, with I well above 0.3, and the shuffled genes
must lie within a few standard deviations of E[I] = -1 / (n - 1).  Then the same question for the factors of a small NMF fit of
the tissue (moran_factors).  Makes no download.  Needs an MI355X.

  python examples/spatial_variable_features.py [side] [genes] [planted]        defaults: 100, 2000, 20
"""
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

side, m, planted = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (100, 2000, 20)
rng = np.random.default_rng(0)
n = side * side
xs, ys = np.arange(n) % side, np.arange(n) // side
which = np.sort(rng.permutation(m)[:planted])
D = np.zeros((m, n))
for g in range(m):
    x0, y0 = rng.integers(0, side // 2, 2)
    w, h = rng.integers(side // 4, side // 2, 2)
    inside = (xs >= x0) & (xs < x0 + w) & (ys >= y0) & (ys < y0 + h)
    D[g] = rng.poisson(np.where(inside, 6.0, 0.3))
    if g not in which:
        D[g] = D[g][rng.permutation(n)]                     # the same values, no spatial pattern
counts = sa.as_dgCMatrix(sparse.csc_matrix(D))
print("tissue: %d x %d grid, %d genes (%d planted), %d non-zeros" % (side, side, m, planted, counts.nnz))

coords = np.stack([xs, ys], axis=1).astype(np.float64)
t0 = time.perf_counter()
res = sa.find_spatially_variable_features(counts, coords=coords, max_dist=1.5, nfeatures=planted)
t1 = time.perf_counter()
print("find_spatially_variable_features: %d genes over %d cells in %.3f s (graph, upload and host statistics included)" % (m, n, t1 - t0))
shuffled = np.setdiff1d(np.arange(m), which)
print("first %d features are the planted genes: %s" % (planted, sorted(res["features"].tolist()) == which.tolist()))
print("planted  genes: I from %.3f to %.3f, largest p_adj %.3g" % (res["I"][which].min(), res["I"][which].max(), res["p_adj"][which].max()))
dev = np.abs(res["I"][shuffled] - res["EI"][shuffled]) / res["sd"][shuffled]
print("shuffled genes: |I - E[I]| / sd at most %.2f, %d of %d with p_adj < 0.05" % (dev.max(), (res["p_adj"][shuffled] < 0.05).sum(), shuffled.size))

# the factors of a fit: spatially coherent factors carry the planted domains
model = sa.run_nmf(counts, 8, maxit=30, verbose=False, seed=1)
graph = sa.spatial_graph(coords[:, 0], coords[:, 1], 1.5, 100)
fac = sa.moran_factors(model, graph)
print("factors of a rank-8 fit: I = %s" % np.round(fac["I"], 3))
