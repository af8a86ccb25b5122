#!/usr/bin/env python3
"""Score six small marker signatures in every cell of the reference's bundled pbmc3k counts (UCell's rank-based score,
score_signatures -> sgl_signature_scores: one descending ordering of every cell's values on the device) and print the mean
score of every signature per bundled cell type.  The score depends only on the order of the values within a cell, so the
raw counts are scored as they are.  Needs an MI355X.

  python examples/pbmc3k_score_signatures.py [max_rank]        default: 1500
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

signatures = {"B": ["CD79A", "MS4A1", "CD79B"], "NK": ["GNLY", "NKG7", "GZMB"], "Platelet": ["PPBP", "PF4"], "DC": ["FCER1A", "CST3"],
              "T": ["CD3D", "CD3E", "CD2"], "Mono": ["LYZ", "CD14", "S100A9", "FCGR3A"]}
max_rank = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
t0 = time.perf_counter()
res = sa.score_signatures(counts, signatures, max_rank=max_rank)      # the gene names are the matrix's row names
t1 = time.perf_counter()
print("score_signatures: %d signatures x %d cells in %.3f s (upload included)" % (len(res["names"]), counts.ncol, t1 - t0))
print("%-10s" % "type" + "".join("%10s" % n for n in res["names"]) + "     cells")
for t in range(1, 10):
    sel = cell_type == t
    print("%-10d" % t + "".join("%10.3f" % res["scores"][sel, j].mean() for j in range(len(res["names"]))) + "%10d" % sel.sum())
for j, n in enumerate(res["names"]):
    mean = np.array([res["scores"][cell_type == t, j].mean() for t in range(1, 10)])
    print("%-9s highest in type %d (%.3f), next %.3f" % (n, mean.argmax() + 1, mean.max(), np.sort(mean)[-2]))
