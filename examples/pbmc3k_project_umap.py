#!/usr/bin/env python3
"""Query cells drawn in a reference's UMAP picture on the reference's bundled pbmc3k counts, every numeric step through
libsinglet_hip.so: hold out the last 700 cells, fit and cluster the first 2 000, lay them out (run_umap, which also returns
the model a later projection needs), then project the held-out cells onto the reference's w (project_model) and place them in
the picture (project_umap: a search against the reference's embedding, memberships, start and all epochs on the device).  The
placement is scored by the share of a query's 15 nearest references in the embedding that are among its 15 nearest in the
picture, beside the score of the start (the neighbour-weighted mean, what transfer_values would give).  Needs an MI355X.

  python examples/pbmc3k_project_umap.py [n_reference]        default: 2000
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
p, dim = g["p"].astype(np.int64), g["dim"]
i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
for c in range(dim[1]):
    i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
x = g["x"].astype(np.float64)
n, n_ref = int(dim[1]), int(sys.argv[1]) if len(sys.argv) > 1 else 2000


def cells(lo, hi):
    return sa.dgCMatrix(x[p[lo]:p[hi]], i[p[lo]:p[hi]].astype(np.int32), (p[lo:hi + 1] - p[lo]).astype(np.int32), (int(dim[0]), hi - lo))


def share(E_ref, E_query, Y_ref, Y_query, k=15):
    ne = sa.knn(E_ref.T, E_query.T, k)[0]
    ny = sa.knn(Y_ref.T, Y_query.T, k)[0]
    return float(np.mean([np.intersect1d(ne[q], ny[q]).size / float(k) for q in range(ne.shape[0])]))


reference, query = sa.PreprocessData(cells(0, n_ref)), sa.PreprocessData(cells(n_ref, n))     # Seurat::LogNormalize, per cell
fit = sa.run_nmf(reference, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
E_ref = np.ascontiguousarray(fit["h"].T)                                                     # cells x factors
t0 = time.perf_counter()
Y_ref, model = sa.run_umap(fit["h"], n_neighbors=30, return_model=True)
t1 = time.perf_counter()
print("reference: %d cells laid out in %.3f s (a = %.4f, b = %.4f)" % (n_ref, t1 - t0, model.a, model.b))

E_query = np.ascontiguousarray(np.asarray(sa.project_model(query, fit["w"])["h"]).T)
t0 = time.perf_counter()
Y_init, Y_query = sa.project_umap(model, E_ref, E_query, return_init=True)
t1 = time.perf_counter()
info = sa.umap_transform_info()
print("%d query cells placed in %.3f s (instance %d, widest list %d, %d without a neighbour, %d launch(es))"
      % (n - n_ref, t1 - t0, info["instance"], info["widest_list"], info["empty_queries"], info["launches"]))
print("share of the 15 nearest references kept in the picture: start %.3f, after the epochs %.3f"
      % (share(E_ref, E_query, Y_ref, Y_init), share(E_ref, E_query, Y_ref, Y_query)))

# the same through a ReferenceIndex that stays on the device for any number of query batches
with sa.ReferenceIndex(E_ref, method="exact", layout=Y_ref) as index:
    out = index.project(E_query, model.a, model.b, model.n_neighbors, alpha0=0.25 * model.learning_rate, seed=model.seed)
print("the kept index gives the same bits:", bool(np.array_equal(out["layout"].view(np.uint64), Y_query.view(np.uint64))))
