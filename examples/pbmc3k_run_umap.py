#!/usr/bin/env python3
"""The clustering vignette's whole pipe (RunNMF %>% FindNeighbors %>% FindClusters %>% RunUMAP(reduction = "nmf")) on the
reference's bundled pbmc3k counts, every numeric step through libsinglet_hip.so: LogNormalize -> run_nmf(rank = 10) ->
run_umap (exact k-NN, fuzzy neighbour graph, synchronous layout) -> find_neighbors, find_clusters for the colours.  With
matplotlib the layout is drawn to pbmc3k_umap.png, coloured by cluster; without it the times are printed.  Needs an MI355X.
--metric cosine (Seurat's RunUMAP default) or correlation searches the neighbours of both steps by direction, not magnitude.

  python examples/pbmc3k_run_umap.py [--metric euclidean|cosine|correlation] [out.png]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

ap = argparse.ArgumentParser(description="pbmc3k: run_nmf, run_umap, find_neighbors, find_clusters on the GPU")
ap.add_argument("--metric", choices=("euclidean", "cosine", "correlation"), default="euclidean", help="metric of the neighbour search")
ap.add_argument("out", nargs="?", default="pbmc3k_umap.png", help="the picture (needs matplotlib)")
opts = ap.parse_args()

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
Y, G = sa.run_umap(fit["h"], n_neighbors=30, min_dist=0.3, return_graph=True, metric=opts.metric)     # k x cells, one column per cell
t1 = time.perf_counter()
clusters = sa.find_clusters(sa.find_neighbors(fit["h"].T, k_param=20, metric=opts.metric), resolution=0.8)["clusters"][:, 0]
t2 = time.perf_counter()
print("run_umap (%s): %d cells, fuzzy graph of %d entries, 500 epochs in %.3f s (kernel instance %d); clusters in %.3f s"
      % (opts.metric, Y.shape[0], G.nnz, t1 - t0, sa.umap_info()["instance"], t2 - t1))
print("layout spans [%.2f, %.2f] x [%.2f, %.2f]; %d clusters" % (Y[:, 0].min(), Y[:, 0].max(), Y[:, 1].min(), Y[:, 1].max(),
                                                                clusters.max() + 1))
try:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
except ImportError:
    print("matplotlib is not installed: no picture")
else:
    out = opts.out
    plt.figure(figsize=(6, 6))
    plt.scatter(Y[:, 0], Y[:, 1], c=clusters, s=3, cmap="tab20")
    plt.xlabel("UMAP 1")
    plt.ylabel("UMAP 2")
    plt.savefig(out, dpi=150)
    print("wrote", out)
