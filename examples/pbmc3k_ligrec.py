#!/usr/bin/env python3
"""Cell-cell communication after the clustering vignette's pipe (RunNMF %>% FindNeighbors %>% FindClusters) on the reference's
bundled pbmc3k counts, every numeric step through libsinglet_hip.so: LogNormalize -> run_nmf(rank = 10) -> find_neighbors ->
find_clusters -> ligrec (the permutation test of CellPhoneDB / squidpy's gr.ligrec under this library's own rules and
relabellings: include/singlet_hip.h, "Ligand-receptor interactions").  The library ships no interaction database: the pairs
below are typed by hand.  The bundled fixture carries no gene names, so they are rows of the matrix -- with names, pass
(ligand, receptor) names and gene_names = the row names, or the path of a two-column TSV file.  Needs an MI355X.

  python examples/pbmc3k_ligrec.py [nperm]        default: 1000
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
clusters = sa.find_clusters(graph, resolution=0.8)["clusters"][:, 0]
K = int(clusters.max()) + 1
print("find_clusters: %d clusters, sizes %s" % (K, np.bincount(clusters).tolist()))

# (ligand row, receptor row): typed by hand; a row may serve many pairs, and a gene may be paired with itself
PAIRS = [(100, 2500), (100, 7300), (2500, 100), (512, 512), (1200, 9000), (4000, 4100), (6100, 12000), (8000, 350), (9000, 1200),
         (11000, 11500), (13000, 100), (350, 8000)]
nperm = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
t0 = time.perf_counter()
res = sa.ligrec(A, clusters, PAIRS, threshold=0.01, nperm=nperm, seed=0)
t1 = time.perf_counter()
print("ligrec: %d pairs x %d x %d cluster pairs, %d relabellings in %.3f s" % (len(res["pairs"]), K, K, nperm, t1 - t0))
tested = ~np.isnan(res["p"])
print("tested (ligand and receptor expressed in >= 1 %% of the class): %d of %d" % (tested.sum(), tested.size))
order = np.argsort(np.where(tested, res["padj"], np.inf), axis=None, kind="stable")[:10]
for flat in order:
    q, a, b = np.unravel_index(flat, res["p"].shape)
    if tested[q, a, b]:
        print("    pair %-14s cluster %d -> %d   mean %.4f   p %.4f   padj %.4f" % (res["pairs"][q], a, b, res["means"][q, a, b], res["p"][q, a, b],
                                                                                res["padj"][q, a, b]))
