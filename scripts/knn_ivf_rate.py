#!/usr/bin/env python3
"""Time the inverted-list neighbour search (Context.knn(method="ivf")) against the exact search on the same data in the same
session, and measure its recall.  Writes one JSON line to profiles/knn_ivf_rate.json (or the path in KNN_IVF_RATE_OUT) and
prints it.

Data.  "clustered": k x cells, a mixture of PROFILES sparse non-negative profiles (a third of the k entries non-zero, uniform
in [0.5, 2)), every cell its profile (drawn by rng.integers) times a per-entry gamma(shape 20, scale 1 / 20) factor and a size
factor uniform in [0.8, 1.25), plus 0.01 gamma(2, 0.5) on every entry; numpy default_rng(SEED).  (The uniform synthetic of
scripts/knn_rate.py has no neighbourhood structure: recall on it would measure nothing.)
"pbmc3k": the H of run_nmf(rank = 15) on the LogNormalized counts of tests/golden/pbmc3k_counts.npz, 2 700 cells.

Per case (the cases of profiles/knn_rate.json: self search of 200 000 x 50, 1 000 000 x 10 and x 50 cells; 1 000 queries
against 1 000 000 x 50; and pbmc3k), n_neighbors = 20, n_lists = ceil(sqrt(cells)) -- the default:
  exact     sgl_knn on the same data: its kernel time (the "scale" phase) and wall time, medians of EXACT_REPEATS after a
            warm-up
  ivf       the whole call at the default n_probe: wall time, the "scale" phase (list scan, merge and the centroid updates)
            and the eight stages (sgl_knn_ivf_stage_ms: events on the stream; the task table is host work, by the host
            clock), medians of REPEATS after a warm-up
  recall    recall@20 against the exact search for n_probe in 1, 2, 4, 8, 16, 32, 64, on a sample of SAMPLE queries in query
            form (the cells themselves as Q), under one training (op_ivf_train, then op_ivf_search per n_probe), with the wall
            time of each search
  default_rule  the smallest power of two whose recall is at least 0.99 in this case
No speed-up is fixed in advance and no test gates on these numbers.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("KNN_IVF_RATE_OUT") or os.path.join(ROOT, "profiles", "knn_ivf_rate.json")
REPEATS = int(os.environ.get("KNN_IVF_RATE_REPEATS", "3"))
EXACT_REPEATS = int(os.environ.get("KNN_IVF_RATE_EXACT_REPEATS", str(REPEATS)))   # the exact search at 10^6 x 50 takes 13 s a call
CASES = os.environ.get("KNN_IVF_RATE_CASES", "pbmc3k,self50-200000,self10-1000000,self50-1000000,query50-1000000").split(",")
SAMPLE = int(os.environ.get("KNN_IVF_RATE_SAMPLE", "10000"))
K, PROFILES, SEED = 20, 64, 20261020
PROBES = (1, 2, 4, 8, 16, 32, 64)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def clustered(k, n):
    rng = np.random.default_rng(SEED)
    profiles = np.where(rng.random((k, PROFILES)) < 1.0 / 3.0, rng.uniform(0.5, 2.0, (k, PROFILES)), 0.0)
    label = rng.integers(0, PROFILES, n)
    X = profiles[:, label] * rng.gamma(20.0, 1.0 / 20.0, (k, n)) * rng.uniform(0.8, 1.25, n)[None, :]
    return X + 0.01 * rng.gamma(2.0, 0.5, (k, n))


def pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    counts = sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))
    fit = sa.run_nmf(sa.PreprocessData(counts), rank=15, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
    return np.ascontiguousarray(fit["h"])


def timed(c, fn, repeats, stages=False):
    kern, wall, st = [], [], []
    for rep in range(repeats + 1):
        c.timing_get(reset=True)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            kern.append(c.timing_get(reset=True)["scale"][0])
            if stages:
                st.append(c.knn_ivf_stage_ms())
    out = {"kernel_ms": stats(kern), "call_wall_ms": stats(wall), "repeats": repeats}
    if stages:
        out["stage_ms"] = {name: float(np.median([s[name] for s in st])) for name in st[0]}
    return out


def measure(sa, case):
    from singlet_amd._marshal import knn_ivf_shape
    if case == "pbmc3k":
        X, form = pbmc3k(sa), "self"
    else:
        form, cells = case.split("-")
        X, form = clustered(int(form.lstrip("selfquery")), int(cells)), form.rstrip("0123456789")
    k, n = X.shape
    rng = np.random.default_rng(1)
    sample = np.sort(rng.choice(n, min(SAMPLE, n), replace=False))
    Qs = np.ascontiguousarray(X[:, sample])
    Q = np.ascontiguousarray(X[:, rng.choice(n, 1000, replace=False)]) if form == "query" else None
    n_lists, n_probe = knn_ivf_shape(n)
    res = {"case": case, "form": form, "k": k, "cells": n, "n_query": n if Q is None else 1000, "n_neighbors": K, "n_lists": n_lists,
           "default_n_probe": n_probe, "sample": int(sample.size)}
    with sa.Context(0) as c:
        c.timing_enable(True)
        res["exact"] = timed(c, lambda: c.knn(K, X, Q), EXACT_REPEATS)
        res["ivf"] = timed(c, lambda: c.knn(K, X, Q, method="ivf", n_lists=n_lists, n_probe=n_probe), REPEATS, stages=True)
        res["ivf"]["report"] = c.knn_ivf_info()
        res["exact_kernel_over_ivf_call"] = res["exact"]["kernel_ms"]["median"] / res["ivf"]["call_wall_ms"]["median"]
        exact_idx = c.knn(K, X, Qs)[0]
        t0 = time.perf_counter()
        cent, assign = c.op_ivf_train(n_lists, X)
        res["train_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        res["recall"] = {}
        for p in PROBES:
            if p > n_lists:
                continue
            t0 = time.perf_counter()
            idx = c.op_ivf_search(cent, assign, p, K, X, Qs)[0]
            wall = 1e3 * (time.perf_counter() - t0)
            res["recall"][str(p)] = {"recall_at_20": sa.knn_recall(idx, exact_idx), "short_queries": c.knn_ivf_info()["short_queries"],
                                     "search_wall_ms": wall}
        ok = [p for p in PROBES if str(p) in res["recall"] and res["recall"][str(p)]["recall_at_20"] >= 0.99]
        res["default_rule"] = min(ok) if ok else None
    return res


def main():
    import singlet_amd as sa
    res = {"repeats": REPEATS, "exact_repeats": EXACT_REPEATS, "sample": SAMPLE, "profiles": PROFILES, "seed": SEED, "cases": []}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for case in CASES:
        res["cases"].append(measure(sa, case))
        with open(OUT, "w") as f:   # after every case: a run cut short keeps what it measured
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res["cases"][-1]), flush=True)
    rules = [c["default_rule"] for c in res["cases"]]
    res["default_n_probe_by_rule"] = None if (not rules or None in rules) else max(rules)
    with open(OUT, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
