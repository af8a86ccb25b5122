#!/usr/bin/env python3
"""Time the signature scores (Context.signature_scores) and their rank stage (Context.op_cell_ranks).  Writes one JSON line to
profiles/signature_rate.json (or the path in SIGNATURE_RATE_OUT) and prints it.

  pbmc3k     the bundled counts (2 700 cells, median 816 stored entries, the longest 3 400): both LDS instances.
  config 3   sgl_synth_csc 30 000 genes x 1 000 000 cells at 5 %: cells of about 1 500 entries, the large LDS instance.
SETS sets of 10 - 200 genes drawn by a fixed generator, max_rank = 1500.  After one warm-up call each, REPEATS timed calls:
the kernels by hipEvent (the "scale" phase, which nothing else of these calls is booked under) and the whole call by the
wall clock (gene -> sets table, count pass and its copy back, kernels, copies of the n_sets x ncol results).  Beside them,
from the same session: the markers' rank pass on the same matrix (it sorts the same entries along the other axis), one
gene-mean pass of the variable features (the bandwidth yardstick: it reads the same 8 + 4 bytes per stored entry), and the
numpy restatement (tests/signature_restatement.py) timed on NUMPY_CELLS cells (pbmc3k: spread over the matrix; config 3: the
first cells of the same generator) and scaled to all of them: the CPU baseline.  The rank stage returns 8 bytes per stored
entry to the host, so it is timed only below RANKS_MAX_NNZ entries.  No time is a pass condition."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.environ.get("SIGNATURE_RATE_OUT", os.path.join(ROOT, "profiles", "signature_rate.json"))
GENES = int(os.environ.get("SIGNATURE_RATE_GENES", "30000"))
CELLS = int(os.environ.get("SIGNATURE_RATE_CELLS", "1000000"))
SETS = int(os.environ.get("SIGNATURE_RATE_SETS", "50"))
REPEATS = int(os.environ.get("SIGNATURE_RATE_REPEATS", "3"))
CLUSTERS = 20
MAX_RANK = 1500
NUMPY_CELLS = 200
RANKS_MAX_NNZ = 200000000


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


def gene_sets(m):
    rng = np.random.default_rng(50)
    return [rng.choice(m, size=int(k), replace=False).astype(np.int32) for k in rng.integers(10, 201, size=SETS)]


def passes(c, sample):
    """sample: (x, i, p), NUMPY_CELLS cells of the matrix (or of one generated like it) for the CPU baseline."""
    import signature_restatement as sr
    m, n, nnz = c.dims()
    sets = gene_sets(m)
    cell = np.arange(n, dtype=np.uint64)
    labels = (((cell * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(CLUSTERS)).astype(np.int32)
    res = {"genes": m, "cells": n, "nnz": nnz, "sets": SETS, "set_genes": int(sum(len(s) for s in sets)), "max_rank": MAX_RANK}
    c.timing_enable(True)
    res["hvg_mean_pass"] = timed(c, c.op_gene_mean)
    res["scores"] = timed(c, lambda: c.signature_scores(sets, MAX_RANK))
    res["paths"] = c.signature_info()
    timed_keys = ["hvg_mean_pass", "scores", "marker_ranks"]
    if nnz <= RANKS_MAX_NNZ:
        res["cell_ranks"] = timed(c, lambda: c.op_cell_ranks(MAX_RANK))
        timed_keys.append("cell_ranks")
    res["marker_ranks"] = timed(c, lambda: c.op_marker_ranks(labels, CLUSTERS))
    res["marker_paths"] = c.markers_info()
    for key in timed_keys:
        res[key]["entries_per_s"] = nnz / (1e-3 * res[key]["kernel_ms"]["median"])
    res["scores"]["cells_per_s"] = n / (1e-3 * res["scores"]["kernel_ms"]["median"])
    res["scores_over_marker_ranks"] = res["scores"]["kernel_ms"]["median"] / res["marker_ranks"]["kernel_ms"]["median"]
    res["scores_over_hvg_pass"] = res["scores"]["kernel_ms"]["median"] / res["hvg_mean_pass"]["kernel_ms"]["median"]
    x, i, p = sample
    t0 = time.perf_counter()
    sr.scores(x, i, p, m, sets, MAX_RANK)
    dt = time.perf_counter() - t0
    cells = len(p) - 1
    res["numpy_restatement"] = {"cells_timed": cells, "entries_timed": int(p[-1]), "wall_s": dt, "scaled_to_all_cells_s": dt * n / cells}
    return res


def pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    counts = sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))
    cells = np.linspace(0, counts.ncol - 1, NUMPY_CELLS).astype(np.int64)
    p = p.astype(np.int64)
    take = np.concatenate([np.arange(p[q], p[q + 1]) for q in cells])
    sample = (counts.x[take], counts.i[take], np.concatenate([[0], np.cumsum(p[cells + 1] - p[cells])]))
    with sa.Context(0) as c:
        c.upload(counts)
        return passes(c, sample)


def config3(sa):
    with sa.Context(0) as c:   # the baseline's cells: the first NUMPY_CELLS of the same generator
        c.synth(GENES, NUMPY_CELLS, 20, ncells_total=CELLS)
        sample = c.download(0)
    with sa.Context(0) as c:
        c.synth(GENES, CELLS, 20)
        return passes(c, sample)


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
