#!/usr/bin/env python3
"""Time the embedding k-NN (Context.knn, find_neighbors) on the resident H of a fit.  Writes one JSON line to
profiles/knn_rate.json (or the path in KNN_RATE_OUT) and prints it.

The embedding is the H of two iterations on sgl_synth_csc GENES x cells at 5 % (its values do not matter to the cost of the
scan, only to how often a candidate enters a list).  Per case, after one warm-up call, REPEATS timed calls: the kernels by
hipEvent (the "scale" phase, which nothing else of these calls is booked under) and the whole call by wall clock (checks,
candidate buffers, kernels, the copy of idx and dist to the host).  n_neighbors = 20.

The bound every case is reported against: 3 n_query n_ref n_dims FP64 VALU lane-operations (sub, mul, add per pair and
dimension; the rule forbids the fused form) over 39.3e12 lane-operations per second -- the vector FP64 rate behind the
78.6 TFLOP/s of the specification sheet, which counts a fused multiply-add as two.  That rate is the specification's, not a
measurement.

Next to it the numpy restatement of the rules (tests/embedding_knn_restatement.py) on one CPU core, in seconds per 1000
queries, measured on RESTATE_QUERIES queries and scaled: a restatement, not a tuned CPU search.

--metric cosine | correlation (sgl_knn_metric): every case is taken twice in the same run and on the same context, under the
Euclidean metric (the kernels of a plain run) and under the given one, and the line goes to profiles/knn_metric_rate.json.
Per case "euclidean" and "metric" hold the kernel and wall times, "unit_ms" the knn_unit pass alone (the "gram" phase, which
nothing else of these calls is booked under), "kernel_ratio" the metric's scan over the Euclidean one.  The metric's bound
is 2 n_query n_ref n_dims lane-operations (mul, add) at the same rate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.environ.get("KNN_RATE_OUT")
GENES = int(os.environ.get("KNN_RATE_GENES", "2000"))
REPEATS = int(os.environ.get("KNN_RATE_REPEATS", "5"))
CASES = os.environ.get("KNN_RATE_CASES", "self50-2700,self50-200000,self50-1000000,self10-1000000,query50-1000000,graph50-200000").split(",")
K, LANE_OPS_PER_S, RESTATE_QUERIES = 20, 39.3e12, 20


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed(c, fn):
    """(kernel ms by hipEvent, wall ms, knn_unit ms) of REPEATS calls of fn after one warm-up."""
    kern, wall, unit = [], [], []
    for rep in range(REPEATS + 1):
        c.timing_get(reset=True)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            t = c.timing_get(reset=True)
            kern.append(t["scale"][0])
            unit.append(t["gram"][0])
    return stats(kern), stats(wall), stats(unit)


def restatement_s_per_1000(H, nq):
    import embedding_knn_restatement as rs
    Q = np.ascontiguousarray(H[:, :nq])
    t0 = time.perf_counter()
    rs.knn(H, Q, K)
    return (time.perf_counter() - t0) * 1000.0 / nq


def measure(sa, case, metric):
    form, cells = case.split("-")
    k, cells = int(form.lstrip("selfquerygraph")), int(cells)
    res = {"case": case, "form": form.rstrip("0123456789"), "k": k, "cells": cells, "n_neighbors": K}
    with sa.Context(0) as c:
        c.synth(GENES, cells, 20)
        c.fit_init(k)
        for _ in range(2):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        c.timing_enable(True)
        n_query = cells
        Q = None
        if res["form"] == "query":
            n_query = 1000
            H = c.get_factors()[2]
            Q = np.ascontiguousarray(H[np.random.default_rng(1).choice(cells, n_query, replace=False)].T)

        def search(m):
            if res["form"] == "graph":
                return timed(c, lambda: sa.find_neighbors(c, k_param=K, metric=m))
            return timed(c, lambda: c.knn(K, None, Q, metric=m))

        kern, wall, _ = search("euclidean")
        res.update(n_query=n_query, kernel_ms=kern, call_wall_ms=wall, plan=c.knn_info())
        if metric != "euclidean":
            mk, mw, unit = search(metric)
            res.update(euclidean={"kernel_ms": res.pop("kernel_ms"), "call_wall_ms": res.pop("call_wall_ms")},
                       metric={"name": metric, "kernel_ms": mk, "call_wall_ms": mw, "unit_ms": unit, "report": c.knn_metric_info()},
                       kernel_ratio=mk["median"] / kern["median"])
            if res["form"] != "graph":
                bound_ms = 1e3 * 2.0 * n_query * cells * k / LANE_OPS_PER_S
                res["metric"].update(bound_ms=bound_ms, fraction_of_bound=bound_ms / mk["median"])
        if res["form"] != "graph":   # (the graph's "scale" time holds the k-NN kernels alone; its wall clock the SNN too)
            bound_ms = 1e3 * 3.0 * n_query * cells * k / LANE_OPS_PER_S
            res.update(bound_ms=bound_ms, fraction_of_bound=bound_ms / kern["median"])
            H = c.get_factors()[2]
            res["restatement_cpu_s_per_1000_queries"] = restatement_s_per_1000(np.ascontiguousarray(H.T), RESTATE_QUERIES)
    return res


def main():
    import singlet_amd as sa
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--metric", choices=("euclidean", "cosine", "correlation"), default="euclidean")
    metric = ap.parse_args().metric
    out = OUT or os.path.join(ROOT, "profiles", "knn_rate.json" if metric == "euclidean" else "knn_metric_rate.json")
    res = {"genes": GENES, "repeats": REPEATS, "lane_ops_per_s_spec": LANE_OPS_PER_S, "restatement_queries": RESTATE_QUERIES, "cases": []}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for case in CASES:
        res["cases"].append(measure(sa, case, metric))
        with open(out, "w") as f:   # after every case: a run cut short keeps what it measured
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res["cases"][-1]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
