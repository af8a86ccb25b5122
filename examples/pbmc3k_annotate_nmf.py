#!/usr/bin/env python3
"""The reference's own pipe, PreprocessData %>% RunNMF %>% AnnotateNMF, on its bundled pbmc3k counts, every numeric step
through libsinglet_hip.so: LogNormalize -> run_nmf(rank = 10) -> find_neighbors -> find_clusters, whose labels stand in for a
metadata column (the bundled counts carry none) -> AnnotateNMF: the means-model fit of every factor against the column on the
device and the table of (group, factor) pairs with positive log-odds.  Needs an MI355X.

  python examples/pbmc3k_annotate_nmf.py [resolution]        default: 0.8
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

meta = {"cluster": np.array(["cluster_%02d" % c for c in clusters]),      # a factor column: kept
        "nCount": np.add.reduceat(np.asarray(counts.x, dtype=np.float64), np.asarray(counts.p[:-1], dtype=np.int64))}   # numeric: not a factor, skipped
print("usable columns:", sa.check_columns(meta))
t0 = time.perf_counter()
annotations = sa.AnnotateNMF(fit, meta)
t1 = time.perf_counter()
table = annotations["cluster"]
print("AnnotateNMF: %d factors x %d groups in %.3f s, %d pairs with positive log-odds" % (fit["h"].shape[0], clusters.max() + 1, t1 - t0, table["fc"].size))
print("%-12s %-8s %10s %12s" % ("group", "factor", "fc (lods)", "p (BH)"))
order = np.lexsort((-table["fc"], table["group"]))
for r in order:
    print("%-12s %-8s %10.2f %12.3e" % (table["group_names"][r], table["factor_names"][r], table["fc"][r], table["p"][r]))

# the same fit, field by field (limma's names), and its two-sided table
labels, levels = sa.get_designs(meta)["cluster"]
fit_c = sa.get_model_fit(labels, len(levels), fit)
print("df.residual %d, s2.prior %.4g, df.prior %.4g, df.total %.6g" % (fit_c["df_residual"], fit_c["s2_prior"], fit_c["df_prior"], fit_c["df_total"]))
both = sa.get_model_results(fit_c, tail="std", names=(levels, fit.get("factor_names")))
print("two-sided: %d pairs with positive log-odds, %d of them with p < 0.01" % (both["fc"].size, int((both["p"] < 0.01).sum())))
