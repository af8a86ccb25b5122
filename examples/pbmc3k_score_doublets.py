#!/usr/bin/env python3
"""Doublet scores of the reference's bundled pbmc3k counts by the scheme of Scrublet (score_doublets): artificial doublets are
made on the device as the sums of the counts of random pairs of cells (sgl_simulate_doublets), pushed through the same
LogNormalize, the same 2 000 variable features and the same NMF projection as the real cells, and every real cell is asked
how many of its nearest neighbours in the joint embedding are artificial.  Prints the score distributions of the observed
and the simulated cells and the mean score per bundled cell type.  Needs an MI355X.

  python examples/pbmc3k_score_doublets.py [rank] [sim_ratio]        defaults: 10, 2.0
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
p, dim = g["p"], g["dim"]
i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
for c in range(dim[1]):
    i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
names = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_names.npz"))
genes, cell_type = [s.decode() for s in names["genes"]], names["cell_type"]          # cell_type: codes 1 .. 9, 0 = NA
counts = sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])), (genes, None))
print("pbmc3k: %d genes x %d cells, %d non-zeros" % (counts.nrow, counts.ncol, counts.nnz))

rank = int(sys.argv[1]) if len(sys.argv) > 1 else 10
sim_ratio = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
kw = dict(rank=rank, nfeatures=2000, sim_ratio=sim_ratio, seed=1, maxit=30)
t0 = time.perf_counter()
try:
    res = sa.score_doublets(counts, **kw)
except ValueError as e:                # the simulated scores do not show two humps: the caller passes a threshold
    print("no automatic threshold (%s); using 0.25" % e)
    res = sa.score_doublets(counts, threshold=0.25, **kw)
t1 = time.perf_counter()
print("score_doublets: %d observed + %d simulated cells, rank %d, k_adj %d, in %.3f s (fit and uploads included)"
      % (counts.ncol, res["sim_scores"].shape[0], rank, res["k_adj"], t1 - t0))
q = [0.05, 0.25, 0.5, 0.75, 0.95]
print("observed  scores, quantiles %s: %s" % (q, np.round(np.quantile(res["scores"], q), 3)))
print("simulated scores, quantiles %s: %s" % (q, np.round(np.quantile(res["sim_scores"], q), 3)))
print("threshold %.3f: %d of %d observed cells (%.1f %%) and %.1f %% of the simulated ones lie above it"
      % (res["threshold"], res["predicted"].sum(), counts.ncol, 100.0 * res["predicted"].mean(),
         100.0 * (res["sim_scores"] > res["threshold"]).mean()))
print("%-6s%12s%12s%8s" % ("type", "mean score", "predicted", "cells"))
for t in range(1, 10):
    sel = cell_type == t
    print("%-6d%12.3f%12d%8d" % (t, res["scores"][sel].mean(), res["predicted"][sel].sum(), sel.sum()))
