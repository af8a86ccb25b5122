#!/usr/bin/env python3
"""The clustering vignette's RunGSEA step (PreprocessData %>% RunNMF %>% RunGSEA) on the reference's bundled pbmc3k counts,
every numeric step through libsinglet_hip.so: LogNormalize -> run_nmf(rank = 10) -> run_gsea (the pre-ranked enrichment test
of every gene set in every factor against a permutation null, on the device).  Needs an MI355X.

  python examples/pbmc3k_run_gsea.py [sets.gmt] [nperm]        default: built-in demonstration sets, nperm = 10000

The fixture names its genes by row number ("g0", "g1", ...), and MSigDB cannot be downloaded here: without a GMT file whose
gene names match, the example makes its own sets -- one from the top 40 genes of every factor (which must come out enriched
in that factor) and 500 random ones (which must not)."""
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
w = np.ascontiguousarray(fit["w"])                    # genes x factors
names = ["g%d" % r for r in range(w.shape[0])]

if len(sys.argv) > 1 and os.path.exists(sys.argv[1]):
    pathways = sa.read_gmt(sys.argv[1])
else:
    rng = np.random.default_rng(1)
    expressed = np.nonzero(w.sum(axis=1) != 0)[0]
    pathways = {"TOP40_OF_FACTOR_%d" % f: [names[r] for r in np.argsort(-w[:, f], kind="stable")[:40]] for f in range(w.shape[1])}
    for q in range(500):
        pathways["RANDOM_%d" % q] = [names[r] for r in rng.choice(expressed, size=int(rng.integers(11, 200)), replace=False)]
nperm = int(sys.argv[2]) if len(sys.argv) > 2 else 10000

t0 = time.perf_counter()
res = sa.run_gsea(w, pathways, names, nperm=nperm)
t1 = time.perf_counter()
print("run_gsea: %d sets x %d factors on %d genes, nperm = %d, in %.3f s" % (len(res["pathways"]), w.shape[1], res["genes"].size, nperm, t1 - t0))
print("%d sets with a BH-adjusted p below 0.01 in some factor" % res["significant"].size)
for f in range(w.shape[1]):
    col = np.where(np.isnan(res["padj"][:, f]), -np.inf, res["padj"][:, f])
    best = np.argsort(-col, kind="stable")[:3]
    print("factor %d: %s" % (f, ", ".join("%s (-log10 padj %.2f, NES %.2f)" % (res["pathways"][j], res["padj"][j, f], res["nes"][j, f]) for j in best)))
