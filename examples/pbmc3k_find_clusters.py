#!/usr/bin/env python3
"""The clustering vignette's pipe (RunNMF %>% FindNeighbors %>% FindClusters) on the reference's bundled pbmc3k counts, every
numeric step through libsinglet_hip.so: LogNormalize -> run_nmf(rank = 10) -> find_neighbors (exact k-NN of the cells in
the embedding and their SNN graph) -> find_clusters (deterministic Louvain on that graph).  Needs an MI355X.

  python examples/pbmc3k_find_clusters.py [resolution ...]        default: 0.4 0.8 1.2
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
print("run_nmf(rank=10): %d iterations" % fit["iter"])

t0 = time.perf_counter()
graph = sa.find_neighbors(fit["h"].T, k_param=20)     # cells x factors, as cell.embeddings; exact.  At 10^5 cells and more:
#                                                       nn_method="ivf" (approximate, as Seurat's annoy; n_lists=, n_probe=)
t1 = time.perf_counter()
resolutions = [float(a) for a in sys.argv[1:]] or [0.4, 0.8, 1.2]
out = sa.find_clusters(graph, resolution=resolutions)
t2 = time.perf_counter()
print("find_neighbors: SNN graph of %d entries in %.3f s; find_clusters at %d resolutions in %.3f s"
      % (graph["snn"].nnz, t1 - t0, len(resolutions), t2 - t1))
for r, gamma in enumerate(resolutions):
    sizes = np.bincount(out["clusters"][:, r])
    print("resolution %.2f: %d clusters after %d levels, Q = %.4f, sizes %s"
          % (gamma, out["n_clusters"][r], out["levels"][r], out["modularity"][r], sizes.tolist()))
