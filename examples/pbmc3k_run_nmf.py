#!/usr/bin/env python3
"""BASELINE config 1 as a user would run it: the reference's bundled pbmc3k counts ->
PreprocessData (LogNormalize, on the device) -> run_nmf(rank = 10) -> project_model, all through
libsinglet_hip.so.  Needs an MI355X.

  python examples/pbmc3k_run_nmf.py
  python examples/pbmc3k_run_nmf.py features     the same fit on the 2 000 genes with the most non-zeros, through RunNMF:
                                                 normalise, subset and fit on one resident matrix
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
t0 = time.perf_counter()
fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
dt = time.perf_counter() - t0
print("run_nmf(rank=10): %d iterations in %.3f s, d = %s" % (fit["iter"], dt, np.round(fit["d"], 1)))
err = sa.evaluate(A, fit, cell_loss=True)                # the full-matrix error of the fit, zeros included
print("evaluate: mse = %.6g over all %d x %d entries; the worst-explained cell carries %.3g of the squared error"
      % (err["mse"], A.nrow, A.ncol, err["cell_loss"].max() / err["sse"]))
proj = sa.project_model(A, fit["w"])
print("project_model: h is %d x %d, relative change vs the fit's h: %.2e"
      % (proj["h"].shape[0], proj["h"].shape[1], np.linalg.norm(proj["h"] - fit["h"]) / np.linalg.norm(fit["h"])))

if "features" in sys.argv[1:]:
    with sa.Context(0) as ctx:                        # non-zeros per gene, counted on the device
        ctx.upload(counts, None)
        per_gene = ctx.col_counts(1)
    features = np.argsort(-per_gene, kind="stable")[:2000]
    t0 = time.perf_counter()
    sub = sa.RunNMF(counts, k=10, features=features, tol=1e-4, maxit=100, verbose=0, L1=0.01, seed=123)
    dt = time.perf_counter() - t0
    print("RunNMF(k=10, features = the 2000 genes with the most non-zeros): w is %d x %d, %d iterations in %.3f s, d = %s"
          % (sub["w"].shape[0], sub["w"].shape[1], sub["iter"], dt, np.round(sub["d"], 1)))
