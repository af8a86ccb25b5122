#!/usr/bin/env python3
"""Reference mapping on the reference's bundled pbmc3k counts, every numeric step through libsinglet_hip.so: fit and cluster
the first 2 000 cells, keep their embedding on the GPU as a ReferenceIndex with the cluster labels on it, then map the other 700
cells -- project_model onto the reference's w, a search against the kept index, the labels voted along the neighbour lists
(map_query).  The transferred labels are compared with the clusters the same cells get when all 2 700 are fitted and clustered
together.  Needs an MI355X.

  python examples/pbmc3k_map_query.py [n_reference]        default: 2000
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


def clusters_of(A):
    fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
    graph = sa.find_neighbors(fit["h"].T, k_param=20)
    return fit, sa.find_clusters(graph, resolution=[0.8])["clusters"][:, 0]


reference, query = sa.PreprocessData(cells(0, n_ref)), sa.PreprocessData(cells(n_ref, n))     # Seurat::LogNormalize, per cell
fit, labels = clusters_of(reference)
print("reference: %d cells, %d clusters of sizes %s" % (n_ref, labels.max() + 1, np.bincount(labels).tolist()))

t0 = time.perf_counter()
with sa.ReferenceIndex(fit["h"].T, labels=labels, metric="cosine") as index:
    t1 = time.perf_counter()
    out = sa.map_query(query, fit["w"], index, n_neighbors=20)
    t2 = time.perf_counter()
    info = index.info()
print("index of %d lists built in %.3f s (%d bytes resident); %d cells mapped in %.3f s"
      % (info["n_lists"], t1 - t0, info["bytes"], n - n_ref, t2 - t1))
print("transferred labels: sizes %s, median winning share %.3f" % (np.bincount(out["predicted"], minlength=labels.max() + 1).tolist(),
                                                                     float(np.median(out["score"]))))

# the same cells in a joint clustering of all 2 700: cluster ids differ between the two runs, so every joint cluster is named
# after the reference cluster most of its REFERENCE cells belong to, and the query cells are scored against that name
_, joint = clusters_of(sa.PreprocessData(cells(0, n)))
table = np.zeros((joint.max() + 1, labels.max() + 1), dtype=np.int64)
np.add.at(table, (joint[:n_ref], labels), 1)
name = table.argmax(axis=1)
agree = float((name[joint[n_ref:]] == out["predicted"]).mean())
print("joint clustering: %d clusters; %.1f %% of the %d mapped cells carry the label their joint cluster is named after"
      % (joint.max() + 1, 100.0 * agree, n - n_ref))
