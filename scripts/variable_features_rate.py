#!/usr/bin/env python3
"""Time the variable-feature selection (Context.variable_features) on a resident matrix of config 3's size.  Writes one JSON
line to profiles/variable_features_rate.json (or the path in HVG_RATE_OUT) and prints it.

On sgl_synth_csc 30 000 genes x 1 000 000 cells at 5 %, once uniform and once skewed (log-normal cell and gene weights,
sigma 0.5 / 1.5: one gene's length dominates its waves): after one warm-up call each, REPEATS timed calls of the three gene
passes and of the trend on their own (the kernels by hipEvent: the "scale" phase, which nothing else of these calls is
booked under) and of the whole call (wall clock: segment table, kernels, host log10 / sort / pow / ranking, copies).
Bytes under the model of a pass: 8 per stored value, the m + 1 offsets of 8 twice (segment and closing kernel), 12 per
segment (its gene, its partial sum written) + 8 per segment read back and 16 per gene (first segment, result) -- against
8 TB/s.  The trend reads 2 x 8 m' bytes of (x, y) that stay in cache: its figure is time alone.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("HVG_RATE_OUT", os.path.join(ROOT, "profiles", "variable_features_rate.json"))
GENES = int(os.environ.get("HVG_RATE_GENES", "30000"))
CELLS = int(os.environ.get("HVG_RATE_CELLS", "1000000"))
REPEATS, NFEATURES, SPAN, SEG, PEAK = 5, 2000, 0.3, 8192, 8.0e12


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed(c, fn):
    """(kernel ms by hipEvent, wall ms) of REPEATS calls of fn after one warm-up."""
    kern, wall = [], []
    for rep in range(REPEATS + 1):
        c.timing_get(reset=True)
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            kern.append(c.timing_get(reset=True)["scale"][0])
    return stats(kern), stats(wall), out


def measure(sa, name, skew):
    res = {"matrix": name}
    with sa.Context(0) as c:
        c.synth(GENES, CELLS, 20, skew=skew)
        m, n, nnz = c.dims()
        counts = c.col_counts(1)
        nseg = int(np.sum((counts + SEG - 1) // SEG))
        res.update(nnz=nnz, longest_gene=int(counts.max()), median_gene=int(np.median(counts)), segments=nseg)
        pass_bytes = 8 * nnz + 2 * 8 * (m + 1) + 20 * nseg + 16 * m
        res["pass_bytes_model"] = pass_bytes
        c.timing_enable(True)
        k_mean, w_mean, (mean, _) = timed(c, c.op_gene_mean)
        k_var, w_var, var = timed(c, lambda: c.op_gene_var(mean))
        live = np.flatnonzero(var > 0)
        lx, ly = np.log10(mean[live]), np.log10(var[live])
        order = np.lexsort((live, lx))
        q = max(min(live.size, 3), int(np.floor(SPAN * live.size)))
        k_trend, w_trend, fit = timed(c, lambda: c.op_loess_direct(lx[order], ly[order], q))
        sd = np.zeros(m)
        sd[live[order]] = np.sqrt(np.power(10.0, fit))
        k_std, w_std, _ = timed(c, lambda: c.op_gene_var_std(mean, sd, float(np.sqrt(n))))
        _, w_all, out = timed(c, lambda: c.variable_features(NFEATURES, SPAN))
        for key, kern, wall in (("mean", k_mean, w_mean), ("variance", k_var, w_var), ("variance_standardized", k_std, w_std)):
            res[key] = {"kernel_ms": kern, "call_wall_ms": wall, "bytes_per_s": pass_bytes / (1e-3 * kern["median"]),
                        "fraction_of_8TBps": pass_bytes / (1e-3 * kern["median"]) / PEAK}
        res["trend"] = {"kernel_ms": k_trend, "call_wall_ms": w_trend, "points": int(live.size), "window": q}
        res["whole_call_wall_ms"] = w_all
        res["features_head"] = [int(g) for g in out["features"][:8]]
    return res


def main():
    import singlet_amd as sa
    uniform = measure(sa, "uniform", None)
    skewed = measure(sa, "skewed (0.5, 1.5)", (0.5, 1.5))
    ratio = {k: skewed[k]["kernel_ms"]["median"] / uniform[k]["kernel_ms"]["median"] for k in ("mean", "variance", "variance_standardized")}
    res = {"genes": GENES, "cells": CELLS, "repeats": REPEATS, "nfeatures": NFEATURES, "span": SPAN, "segment": SEG,
           "uniform": uniform, "skewed": skewed, "skewed_over_uniform_kernel": ratio}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
