#!/usr/bin/env python3
"""Time a search and a map against a neighbour index kept on the device (Context.knn_index_build / knn_index_search /
knn_index_map) against the one-shot calls with the same references and queries, in one session.  Writes one JSON line to
profiles/knn_index_rate.json (or the path in KNN_INDEX_RATE_OUT) and prints it.

Data: the clustered synthetic of scripts/knn_ivf_rate.py, CELLS x 50 (10^6 by default); the queries are N_QUERY (1 000 and
10 000) of its cells, drawn by default_rng(1).  n_neighbors = 20, n_lists = ceil(sqrt(cells)) and n_probe at their defaults.
  build       the index built once: wall time, and what sgl_knn_index_info reports (the bytes resident among it)
  search      knn_index_search against the kept index: wall time
  map         knn_index_map with 32 classes and 2 values on the index: wall time
  one_shot_ivf, one_shot_exact   sgl_c_knn_ivf and sgl_c_knn with the same queries: wall time -- the baseline, as measured here
  equal       the index search gave the bits of the one-shot inverted-list call
All times are medians of REPEATS calls after a warm-up call.  No test gates on these numbers."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.environ.get("KNN_INDEX_RATE_OUT") or os.path.join(ROOT, "profiles", "knn_index_rate.json")
REPEATS = int(os.environ.get("KNN_INDEX_RATE_REPEATS", "3"))
CELLS = int(os.environ.get("KNN_INDEX_RATE_CELLS", "1000000"))
N_QUERY = [int(v) for v in os.environ.get("KNN_INDEX_RATE_QUERIES", "1000,10000").split(",")]
K, RANK, CLASSES, VALUES = 20, 50, 32, 2


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
    from knn_ivf_rate import clustered
    from singlet_amd._marshal import knn_ivf_shape
    X = clustered(RANK, CELLS)
    n_lists, n_probe = knn_ivf_shape(CELLS)
    rng = np.random.default_rng(1)
    labels = rng.integers(0, CLASSES, CELLS).astype(np.int32)
    values = rng.standard_normal((VALUES, CELLS))
    res = {"k": RANK, "cells": CELLS, "n_neighbors": K, "n_lists": n_lists, "n_probe": n_probe, "classes": CLASSES, "values": VALUES,
           "repeats": REPEATS, "queries": []}
    with sa.Context(0) as c:
        t0 = time.perf_counter()
        c.knn_index_build(X, None, "euclidean", "ivf", n_lists)
        res["build_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        c.knn_index_annotate(labels, CLASSES, values)
        res["annotate_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        res["index"] = c.knn_index_info()
        for nq in N_QUERY:
            Q = np.ascontiguousarray(X[:, rng.choice(CELLS, nq, replace=False)])
            row = {"n_query": nq}
            row["search"], got = wall(lambda: c.knn_index_search(Q, K))
            row["map"], _ = wall(lambda: c.knn_index_map(Q, K))
            row["short_queries"] = c.knn_index_info()["last_short_queries"]
            row["one_shot_ivf"], ivf = wall(lambda: sa.knn(X, Q, K, method="ivf", n_lists=n_lists, n_probe=n_probe))
            row["one_shot_exact"], exact = wall(lambda: sa.knn(X, Q, K))
            row["equal"] = bool(np.array_equal(got[0], ivf[0]) and np.array_equal(got[1], ivf[1]))
            row["recall_at_20"] = sa.knn_recall(got[0], exact[0])
            # the kernels' share of a search and of a map, by the phase events, in calls of their own (timing adds synchronisations)
            c.timing_enable(True)
            for name, fn in (("search", lambda: c.knn_index_search(Q, K)), ("map", lambda: c.knn_index_map(Q, K))):
                fn()
                c.timing_get(reset=True)
                fn()
                t = c.timing_get(reset=True)
                row[name + "_phase_ms"] = {"scale": t["scale"][0], "gram": t["gram"][0]}
            c.timing_enable(False)
            row["one_shot_ivf_over_search"] = row["one_shot_ivf"]["median"] / row["search"]["median"]
            row["one_shot_exact_over_search"] = row["one_shot_exact"]["median"] / row["search"]["median"]
            res["queries"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
