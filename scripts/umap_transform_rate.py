#!/usr/bin/env python3
"""Time the layout transform (Context.knn_index_project, umap_transform, op_umap_transform_epochs) against a neighbour index
kept on the device, in one session.  Writes one JSON line to profiles/umap_transform_rate.json (or the path in
UMAP_TRANSFORM_RATE_OUT) and prints it.

Data: the clustered synthetic of scripts/knn_ivf_rate.py and profiles/knn_index_rate.json, CELLS x 50 (10^6 by default), a
2-D layout of the references drawn at random (the transform's cost does not depend on what the layout shows), 20 neighbours,
n_lists = ceil(sqrt(cells)) and n_probe at their defaults (8 of 1 000 lists); the queries are N_QUERY (1 000, 10 000 and
100 000) of its cells, drawn by default_rng(1).  a, b of min_dist = 0.3, five negative samples, n_epochs at the default (100
up to 10 000 queries, 30 above).
  project         knn_index_project whole (search, memberships, start, transform, downloads): wall time
  map             knn_index_map whole on the same index (32 classes, 2 values): wall time
  stage_whole     op_umap_transform_epochs for all epochs from given W and start -- upload, validation, ONE launch, download
  stage_1_epoch   the same call for epoch 1 alone; (stage_whole - stage_1_epoch) / (n_epochs - 1) is the kernel's time per
                  epoch, and over the terms of an average epoch (the sum of the memberships x 6) the time per term, to be set
                  beside the layout's 0.044 ns (profiles/umap_rate.json)
  stage_launch_per_epoch   stage_whole with SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH=1: the same epochs, one launch each, the
                  position written and read back between them -- the number that says whether the single launch earns its place
  numpy_ms        the numpy restatement of the epochs on the host (1 000 queries only)
All times are medians of REPEATS calls after a warm-up call, in ms.  No test gates on these numbers."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.environ.get("UMAP_TRANSFORM_RATE_OUT") or os.path.join(ROOT, "profiles", "umap_transform_rate.json")
REPEATS = int(os.environ.get("UMAP_TRANSFORM_RATE_REPEATS", "3"))
CELLS = int(os.environ.get("UMAP_TRANSFORM_RATE_CELLS", "1000000"))
N_QUERY = [int(v) for v in os.environ.get("UMAP_TRANSFORM_RATE_QUERIES", "1000,10000,100000").split(",")]
K, RANK, CLASSES, VALUES, NEG, SEED = 20, 50, 32, 2, 5, 42
SWITCH = "SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH"


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def wall(fn, repeats=REPEATS):
    out, last = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        last = fn()
        if rep:
            out.append(1e3 * (time.perf_counter() - t0))
    return stats(out), last


def main():
    import singlet_amd as sa
    import umap_transform_restatement as tr
    from knn_ivf_rate import clustered
    from singlet_amd._marshal import knn_ivf_shape
    X = clustered(RANK, CELLS)
    n_lists, n_probe = knn_ivf_shape(CELLS)
    rng = np.random.default_rng(1)
    labels = rng.integers(0, CLASSES, CELLS).astype(np.int32)
    values = rng.standard_normal((VALUES, CELLS))
    Yref = rng.standard_normal((CELLS, 2)) * 10.0
    a, b = sa.find_ab_params(1.0, 0.3)
    res = {"k": RANK, "cells": CELLS, "n_neighbors": K, "n_lists": n_lists, "n_probe": n_probe, "dim": 2, "a": a, "b": b, "neg_rate": NEG,
           "repeats": REPEATS, "layout_ns_per_term": 0.044, "queries": []}
    with sa.Context(0) as c:
        c.knn_index_build(X, None, "euclidean", "ivf", n_lists)
        c.knn_index_annotate(labels, CLASSES, values)
        c.knn_index_set_layout(Yref.T)
        res["index"] = c.knn_index_info()
        for nq in N_QUERY:
            Q = np.ascontiguousarray(X[:, rng.choice(CELLS, nq, replace=False)])
            n_epochs = 100 if nq <= 10000 else 30
            row = {"n_query": nq, "n_epochs": n_epochs}
            row["project"], out = wall(lambda: c.knn_index_project(Q, a, b, K, None, n_epochs, 0.25, NEG, SEED))
            row["info"] = sa.umap_transform_info()
            row["map"], _ = wall(lambda: c.knn_index_map(Q, K))
            row["short_queries"] = c.knn_index_info()["last_short_queries"]
            row["project_over_map"] = row["project"]["median"] / row["map"]["median"]
            idx, dist = out["idx"], out["dist"]
            W, _, _ = sa.fuzzy_query(idx, dist, CELLS)
            Y0 = out["layout_init"]
            live = (idx >= 0).any(axis=1)
            if not live.all():                      # the stage operator reads no start of a query without a valid slot
                Y0 = np.where(live[:, None], Y0, 0.0)
            stage = lambda t_last: sa.op_umap_transform_epochs(idx, W, Yref, Y0, a, b, n_epochs, 1, t_last, 0.25, NEG, SEED)  # noqa: E731
            row["stage_whole"], whole = wall(lambda: stage(n_epochs))
            row["stage_1_epoch"], _ = wall(lambda: stage(1))
            os.environ[SWITCH] = "1"
            row["stage_launch_per_epoch"], cut = wall(lambda: stage(n_epochs))
            row["launches_with_the_switch"] = sa.umap_transform_info()["launches"]
            del os.environ[SWITCH]
            row["equal_bits_under_the_cut"] = bool(np.array_equal(whole.view(np.uint64), cut.view(np.uint64)))
            row["equal_bits_project_and_stage"] = bool(np.array_equal(whole[live].view(np.uint64), out["layout"][live].view(np.uint64)))
            per_epoch = (row["stage_whole"]["median"] - row["stage_1_epoch"]["median"]) / (n_epochs - 1)
            terms = float(W[W >= 1.0 / n_epochs].sum()) * (1 + NEG)
            row.update({"kernel_per_epoch_ms": per_epoch, "kernel_all_epochs_ms": per_epoch * n_epochs, "terms_per_epoch": terms,
                        "firing_slots_per_query_and_epoch": terms / (1 + NEG) / nq, "ns_per_term": 1e6 * per_epoch / max(terms, 1.0),
                        "launch_per_epoch_minus_one_launch_ms": row["stage_launch_per_epoch"]["median"] - row["stage_whole"]["median"]})
            if nq <= 1000:
                t0 = time.perf_counter()
                tr.epochs(idx, W, Yref, Y0, a, b, n_epochs, 0.25, NEG, SEED)
                row["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            res["queries"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
