#!/usr/bin/env python3
"""The clustering vignette's pipe with the step every user takes next (RunNMF %>% FindNeighbors %>% FindClusters %>%
FindAllMarkers) on the reference's bundled pbmc3k counts, every numeric step through libsinglet_hip.so: LogNormalize ->
run_nmf(rank = 10) -> find_neighbors -> find_clusters -> find_all_markers (the one-vs-rest Wilcoxon rank-sum test of every
gene against every cluster, from one ordering of each gene's values on the device).  Needs an MI355X.

  python examples/pbmc3k_find_markers.py [resolution]        default: 0.8
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
counts = sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))
print("pbmc3k: %d genes x %d cells, %d non-zeros" % (counts.nrow, counts.ncol, counts.nnz))

A = sa.PreprocessData(counts)                         # Seurat::LogNormalize
fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
graph = sa.find_neighbors(fit["h"].T, k_param=20)     # cells x factors, as cell.embeddings
resolution = float(sys.argv[1]) if len(sys.argv) > 1 else 0.8
clusters = sa.find_clusters(graph, resolution=resolution)["clusters"][:, 0]
print("find_clusters(resolution = %.2f): %d clusters, sizes %s" % (resolution, clusters.max() + 1, np.bincount(clusters).tolist()))

t0 = time.perf_counter()
tables = sa.find_all_markers(A, clusters, only_pos=True)
t1 = time.perf_counter()
print("find_all_markers: %d genes x %d clusters tested in %.3f s" % (A.nrow, len(tables), t1 - t0))
for t in tables:
    print("cluster %d: %d markers" % (t["cluster"], t["gene"].size))
    for r in range(min(5, t["gene"].size)):
        print("    gene %6d  p_val %.3e  avg_log2FC %6.3f  pct.1 %.3f  pct.2 %.3f  p_val_adj %.3e"
              % (t["gene"][r], t["p_val"][r], t["avg_log2FC"][r], t["pct_1"][r], t["pct_2"][r], t["p_val_adj"][r]))

# FindMarkers(ident.1 = 0, ident.2 = 1): the two largest clusters against each other
pair = sa.find_markers(A, np.nonzero(clusters == 0)[0], np.nonzero(clusters == 1)[0])
print("find_markers(0 vs 1): %d genes pass the filters" % pair["gene"].size)
