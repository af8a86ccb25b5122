#!/usr/bin/env python3
"""Time the two device passes of the marker genes (Context.op_marker_sums, Context.op_marker_ranks) and the whole call
(Context.markers).  Writes one JSON line to profiles/markers_rate.json (or the path in MARKERS_RATE_OUT) and prints it.

  config 3   sgl_synth_csc 30 000 genes x 1 000 000 cells at 5 %, LogNormalized, 20 clusters dealt out by a hash of the cell:
             every gene is long (about 50 000 stored entries), so the rank pass is the scratch path alone.
  pbmc3k     the bundled counts, LogNormalized, the clusters of the vignette's pipe (run_nmf rank 10 -> find_neighbors ->
             find_clusters): almost every gene sorts in LDS.
After one warm-up call each, REPEATS timed calls: the kernels by hipEvent (the "scale" phase, which nothing else of these
calls is booked under; for the rank pass it spans the batches, the segmented sort and the host's waits between them
included) and the whole call by the wall clock (segment table, label upload, kernels, copies of the m x G results).  Beside
them one gene-mean pass of the variable features from the same session: the bandwidth yardstick of the sums pass, which reads
the same 8 + 4 bytes per stored entry plus the gathered label.  On pbmc3k the same tests by scipy.stats.mannwhitneyu on the
host, timed on SCIPY_GENES genes spread over the matrix and scaled to all of them: the CPU baseline.  No time is a pass
condition."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("MARKERS_RATE_OUT", os.path.join(ROOT, "profiles", "markers_rate.json"))
GENES = int(os.environ.get("MARKERS_RATE_GENES", "30000"))
CELLS = int(os.environ.get("MARKERS_RATE_CELLS", "1000000"))
CLUSTERS = int(os.environ.get("MARKERS_RATE_CLUSTERS", "20"))
REPEATS = int(os.environ.get("MARKERS_RATE_REPEATS", "3"))
SCIPY_GENES = 300


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed(c, fn):
    """(kernel ms by hipEvent, wall ms) of REPEATS calls of fn after one warm-up."""
    kern, wall = [], []
    for rep in range(REPEATS + 1):
        c.timing_get(reset=True)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            kern.append(c.timing_get(reset=True)["scale"][0])
        print("  call %d: %.1f ms" % (rep, 1e3 * (t1 - t0)), file=sys.stderr, flush=True)
    return {"kernel_ms": stats(kern), "call_wall_ms": stats(wall)}


def passes(c, labels, G):
    m, n, nnz = c.dims()
    res = {"genes": m, "cells": n, "nnz": nnz, "clusters": G}
    c.timing_enable(True)
    res["hvg_mean_pass"] = timed(c, c.op_gene_mean)
    res["sums_expm1"] = timed(c, lambda: c.op_marker_sums(labels, G, "expm1"))
    res["sums_identity"] = timed(c, lambda: c.op_marker_sums(labels, G, "identity"))
    res["ranks"] = timed(c, lambda: c.op_marker_ranks(labels, G))
    res["paths"] = c.markers_info()
    res["markers_whole_call"] = timed(c, lambda: c.markers(labels, G))
    for key in ("hvg_mean_pass", "sums_expm1", "sums_identity", "ranks"):
        res[key]["entries_per_s"] = nnz / (1e-3 * res[key]["kernel_ms"]["median"])
    res["sums_over_hvg_pass"] = res["sums_expm1"]["kernel_ms"]["median"] / res["hvg_mean_pass"]["kernel_ms"]["median"]
    return res


def pbmc3k(sa):
    from scipy import sparse, stats as st
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    counts = sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))
    A = sa.PreprocessData(counts)
    fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
    clusters = sa.find_clusters(sa.find_neighbors(fit["h"].T, k_param=20), resolution=0.8)["clusters"][:, 0].astype(np.int32)
    G = int(clusters.max()) + 1
    with sa.Context(0) as c:
        c.upload(A)
        res = passes(c, clusters, G)
    S = sparse.csc_matrix((A.x, A.i, A.p), shape=(A.nrow, A.ncol)).tocsr()
    genes = np.linspace(0, A.nrow - 1, SCIPY_GENES).astype(np.int64)
    t0 = time.perf_counter()
    for gi in genes:
        row = np.asarray(S[gi].todense()).ravel()
        for cl in range(G):
            st.mannwhitneyu(row[clusters == cl], row[clusters != cl], use_continuity=True, alternative="two-sided", method="asymptotic")
    dt = time.perf_counter() - t0
    res["scipy_mannwhitneyu"] = {"genes_timed": int(genes.size), "tests_timed": int(genes.size) * G, "wall_s": dt,
                                 "scaled_to_all_genes_s": dt * A.nrow / genes.size}
    return res


def config3(sa):
    with sa.Context(0) as c:
        c.synth(GENES, CELLS, 20)
        c.log_normalize()
        cell = np.arange(CELLS, dtype=np.uint64)
        labels = ((cell * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(CLUSTERS)
        return passes(c, labels.astype(np.int32), CLUSTERS)


def main():
    import singlet_amd as sa
    res = {"repeats": REPEATS, "pbmc3k": pbmc3k(sa), "config3": config3(sa)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
