#!/usr/bin/env python3
"""Which clusters sit next to which in a synthetic tissue (nhood_enrichment): a grid of cells with planted regions -- two cell
types interleaved like a checkerboard in the left half, a third type filling the right half, and a fourth scattered at random
over everything.  The graph is spatial_graph of the grid coordinates.  The interleaved types must come out as neighbours far
more often than under a random relabelling (z >> 0), both must avoid the block type (z << 0), the block type keeps to itself,
and the scattered type is indifferent to all (|z| of a few).  Makes no download.  Needs an MI355X.

  python examples/spatial_neighbourhood_enrichment.py [side] [nperm]        defaults: 200, 1000
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

side, nperm = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (200, 1000)
rng = np.random.default_rng(0)
n = side * side
xs, ys = np.arange(n) % side, np.arange(n) // side
labels = np.where(xs >= side // 2, 2, (xs + ys) % 2)
labels = np.where(rng.random(n) < 0.1, 3, labels).astype(np.int32)         # the scattered type
names = ["checker A", "checker B", "block", "scattered"]
print("tissue: %d x %d grid, class sizes %s" % (side, side, np.bincount(labels).tolist()))

coords = np.stack([xs, ys], axis=1).astype(np.float64)
t0 = time.perf_counter()
res = sa.nhood_enrichment(labels, coords=coords, max_dist=1.5, nperm=nperm, seed=0)
t1 = time.perf_counter()
print("nhood_enrichment: %d cells, %d counted graph entries, %d permutations in %.3f s (graph, upload and host statistics included)"
      % (n, int(res["counts"].sum()), nperm, t1 - t0))
print("z (rows: the centre cell's class, columns: the neighbour's):")
print("%12s %s" % ("", " ".join("%10s" % s for s in names)))
for a, s in enumerate(names):
    print("%12s %s" % (s, " ".join("%10.1f" % v for v in res["zscore"][a])))
z = res["zscore"]
print("interleaved types are neighbours: %s; both avoid the block: %s; the block keeps to itself: %s; the scattered type is indifferent: %s"
      % (z[0, 1] > 10, z[0, 2] < -10 and z[1, 2] < -10, z[2, 2] > 10, bool(np.abs(z[3]).max() < 5)))
graph = sa.spatial_graph(coords[:, 0], coords[:, 1], 1.5, 100)
print("interaction matrix, rows normalised:")
print(np.round(sa.interaction_matrix(labels, graph, normalized=True), 3))
